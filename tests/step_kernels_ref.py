"""float64 references of the training step's model-free kernels: the Philox words behind the step's uniform and mixture
draws, the epilogues of the unfused loss terms (cnf_score_residual, cnf_rkl_residual), Adam and the loss combiner.  Each
is a restatement of a few lines in NumPy; test_step_kernels_ref_cpu.py checks the restatements themselves (adjoints
against central differences), test_gpu_step_kernels.py holds the kernels to them.  Test helper: no tests here, no GPU."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np

import oracle
from oracle import losses as ol

DRIFT_CODES = {None: -1, "ou": 0, "gradient": 1, "nongradient": 2, "lorenz": 3}      # CnfDrift; -1: no drift


# ---- the draws ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def _philox_words_cached(key, first, n, stream):
  lib = oracle.load_library()
  fn = lib.cnf_oracle_philox4x32
  b0, b1 = first >> 2, (first + n - 1) >> 2
  blk = np.arange(b0, b1 + 1, dtype=np.uint64)
  ctr = np.zeros((blk.size, 4), dtype=np.uint32)
  ctr[:, 0] = (blk & np.uint64(0xFFFFFFFF)).astype(np.uint32)
  ctr[:, 1] = (blk >> np.uint64(32)).astype(np.uint32)
  ctr[:, 2] = stream
  out = np.empty((blk.size, 4), dtype=np.uint32)
  k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], dtype=np.uint32)
  pc, po, pk = ctr.ctypes.data, out.ctypes.data, ctypes.c_void_p(k.ctypes.data)
  vp = ctypes.c_void_p
  for i in range(blk.size):
    fn(vp(pc + 16 * i), pk, vp(po + 16 * i))
  off = first - (b0 << 2)
  words = out.reshape(-1)[off:off + n].copy()
  words.setflags(write=False)
  return words


def philox_words(key, first, n, stream):
  """uint32 [n]: word e & 3 of the Philox4x32-10 block e >> 2 for e = first + i, counter (blk lo, blk hi, stream, 0),
  key (lo, hi) of the 64-bit key -- through cnf_oracle_philox4x32.  Read-only (cached)."""
  if n == 0:
    return np.empty(0, dtype=np.uint32)
  return _philox_words_cached(int(key), int(first), int(n), int(stream))


def uniform24(key, first, n):
  """The step's uniforms (stream 1): the top 24 bits of the word, in [0, 1), float64 (exact)"""
  return (philox_words(key, first, n, 1) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def component(key, first, n):
  """The mixture component of sample first + i (stream 2): the top 3 bits of the word; indexes
  oracle.losses.MIXTURE_CENTERS"""
  return (philox_words(key, first, n, 2) >> np.uint32(29)).astype(np.int64)


# ---- the score terms' epilogue --------------------------------------------------------------------------------------
def drift_jacobian(drift, r3, a):
  """J[i, d, e] = d drift_d / d r_e at r3[i], closed form of oracle.losses.drift (applications.py:310, 353-372)"""
  n, D = r3.shape
  J = np.zeros((n, D, D))
  if drift is None:
    return J
  if drift == "ou":                       # -a r
    J[:, np.arange(D), np.arange(D)] = -a
  elif drift == "gradient":               # a (-(q) x, -(q) y - 2 (y - 1)), q = x^2 + y^2 - 4
    x, y = r3[:, 0], r3[:, 1]
    q = x * x + y * y - 4.0
    J[:, 0, 0] = -a * (q + 2 * x * x)
    J[:, 0, 1] = J[:, 1, 0] = -a * 2 * x * y
    J[:, 1, 1] = -a * (q + 2 * y * y + 2.0)
  elif drift == "nongradient":            # (-a x - y / 2, -a y + x / 2)
    J[:, 0, 0] = J[:, 1, 1] = -a
    J[:, 0, 1] = -0.5
    J[:, 1, 0] = 0.5
  elif drift == "lorenz":                 # (10 (y - x), 28 x - 9 x z - y, 9 x y - 8 z / 3)
    x, y, z = r3[:, 0], r3[:, 1], r3[:, 2]
    J[:, 0, 0], J[:, 0, 1] = -10.0, 10.0
    J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = 28.0 - 9.0 * z, -1.0, -9.0 * x
    J[:, 2, 0], J[:, 2, 1], J[:, 2, 2] = 9.0 * y, 9.0 * x, -8.0 / 3.0
  else:
    raise ValueError(drift)
  return J


def score_residual_u(r, score, n, D, dt, coef, drift, a):
  """u [n, D] = (r2 - r1) / dt + coef score - drift(r3), r = [r1 | r2 | r3]"""
  r = np.asarray(r, dtype=np.float64).reshape(3, n, D)
  u = (r[1] - r[0]) / dt + coef * np.asarray(score, dtype=np.float64).reshape(n, D)
  return u - ol.drift(drift, r[2], a) if drift is not None else u


def slice_sums(v, count):
  """sums [ceil(n / count)] of v [n] over consecutive slices of `count` (the last may be short)"""
  n = v.shape[0]
  n_slices = -(-n // count)
  pad = np.zeros(n_slices * count)
  pad[:n] = v
  return pad.reshape(n_slices, count).sum(1)


def score_residual_ref(r, score, n, count, D, dt, coef, drift, a, loss_coef):
  """(sums [ceil(n / count)], rbar [3 n, D], sbar [n, D]): sums[s] = sum over slice s of |u|^2 and the adjoints of
  loss_coef sum |u|^2 with respect to r and score"""
  r = np.asarray(r, dtype=np.float64).reshape(3 * n, D)
  u = score_residual_u(r, score, n, D, dt, coef, drift, a)
  ub = 2.0 * loss_coef * u
  rbar3 = -np.einsum("id,ide->ie", ub, drift_jacobian(drift, r[2 * n:], a))
  return slice_sums((u * u).sum(1), count), np.concatenate([-ub / dt, ub / dt, rbar3]), coef * ub


# ---- the reverse-KL epilogue ----------------------------------------------------------------------------------------
def rkl_logmix(y, t, T, beta):
  """log(N(y; 0, vs I) (T - t) / T + N(y; 0, vt I) t / T), the mixture formed linearly as reverse_kl_loss_fn forms it
  (-inf where both densities underflow), and the two weighted densities"""
  y = np.asarray(y, dtype=np.float64)
  ps = ol._mvn_iso_pdf(y, 2.0 / beta * (T + 1.0)) * ((T - t) / T)
  pt = ol._mvn_iso_pdf(y, 2.0 / beta) * (t / T)
  with np.errstate(divide="ignore"):
    return np.log(ps + pt), ps, pt


def rkl_residual_ref(y, lp, t, T, beta, loss_coef):
  """(sum, ybar [n, D], lpbar [n]): sum_i lp_i - logmix_i and the adjoints of loss_coef times it"""
  y = np.asarray(y, dtype=np.float64)
  logmix, ps, pt = rkl_logmix(y, t, T, beta)
  vs, vt = 2.0 / beta * (T + 1.0), 2.0 / beta
  with np.errstate(invalid="ignore", divide="ignore"):
    g = (ps / vs + pt / vt) / (ps + pt)                      # -(d logmix / d y_e) / y_e
  return (np.asarray(lp, dtype=np.float64) - logmix).sum(), loss_coef * g[:, None] * y, np.full(y.shape[0], loss_coef)


# rows placed by hand next to the spline range's end (|y_d| = 9.5 of +-10), per dimension: as many far coordinates as
# keep both densities representable in float64 at beta = 10 (|y|^2 / (2 vt) < 700: |y|^2 < 280)
def rkl_far_rows(D):
  rows = np.zeros((6, D))
  rows[0, 0] = 9.5
  rows[1, D - 1] = -9.5
  rows[2, 0] = 9.2
  rows[3, :] = 9.5 / np.sqrt(D)
  rows[4, 0], rows[4, D - 1] = -9.5, 1.0 if D > 1 else -9.5
  rows[5, : min(D, 2)] = 9.5
  return rows.astype(np.float32)


# ---- Adam and the loss combiner -------------------------------------------------------------------------------------
def adam_ref(p, g, mu, nu, lr, b1, b2, eps, step):
  """optax.adam in float64 on the widened float32 inputs: (p, mu, nu) after step `step` (>= 1).  Hyper-parameters are
  taken as the float32 values the kernel receives."""
  p, g, mu, nu = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (p, g, mu, nu))
  lr, b1, b2, eps = (float(np.float32(v)) for v in (lr, b1, b2, eps))
  m = b1 * mu + (1.0 - b1) * g
  v = b2 * nu + (1.0 - b2) * g * g
  bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
  return p - lr * (m / bc1) / (np.sqrt(v / bc2) + eps), m, v


def adam_bounds(p, g, mu, nu, lr, b1, b2, eps, step):
  """adam_ref's (p', mu', nu') and the float32 rounding bounds (bound_p, bound_mu, bound_nu) a kernel's results are held
  to, with EPS = 2^-24 the relative error of one float32 rounding.
  mu' = b1 mu + (1 - b1) g: two products and a sum (1 - b is exact in float32 for b in [1/2, 1)):
  |d mu'| <= 3 EPS (|b1 mu| + |(1 - b1) g|); nu' has one more product and only non-negative terms: |d nu'| <= 4 EPS nu'.
  The update U = lr (mu' / c1) / (sqrt(nu' / c2) + eps), c_i = 1 - b_i^t: powf is good to an ulp of b^t, at most
  2^-23 b^t, so c_i carries rho_i = 2^-23 b_i^t / (1 - b_i^t) relative (the cancellation of 1 - b^t).  sqrt halves nu''s
  4 EPS, rho_2 and the quotient's EPS and adds its own; the sum with eps, mu' / c1, the product with lr and the last
  quotient round once each:
      |dU| <= lr |d mu'| / (c1 (sqrt(nu' / c2) + eps)) + |U| (rho_1 + rho_2 / 2 + 8 EPS),
  and the new parameter rounds once more: |dp| <= |dU| + EPS max(|p|, |p'|) (half an ulp).  mu' = 0 makes U = 0 and
  the parameter exact.  Also returned: (rho_1, rho_2)."""
  EPS = 2.0 ** -24
  want_p, want_mu, want_nu = adam_ref(p, g, mu, nu, lr, b1, b2, eps, step)
  lrf, b1f, b2f, epsf = (float(np.float32(v)) for v in (lr, b1, b2, eps))
  p64, g64, mu64, nu64 = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (p, g, mu, nu))
  bound_mu = 3 * EPS * (np.abs(b1f * mu64) + np.abs((1 - b1f) * g64))
  bound_nu = 4 * EPS * want_nu
  c1, c2 = 1 - b1f ** step, 1 - b2f ** step
  rho1, rho2 = 2 * EPS * b1f ** step / c1, 2 * EPS * b2f ** step / c2
  den = np.sqrt(want_nu / c2) + epsf
  upd = np.abs(p64 - want_p)
  bound_p = lrf * bound_mu / (c1 * den) + upd * (rho1 + rho2 / 2 + 8 * EPS) + EPS * np.maximum(np.abs(p64), np.abs(want_p))
  return (want_p, want_mu, want_nu), (bound_p, bound_mu, bound_nu), (rho1, rho2)


def worst_ratio(e, b):
  """max e / b, a zero bound allowing no error (inf where e > 0 there)"""
  with np.errstate(invalid="ignore", divide="ignore"):
    return float(np.nanmax(np.where(b > 0, e / b, np.where(e > 0, np.inf, 0.0))))


def weighted_sum_ref(v, w):
  """(math.fsum of the exact products v_i w_i, each as its rounded value and the exact remainder; sum_i |v_i w_i|)"""
  terms = []
  for a, b in zip(np.asarray(v, dtype=np.float64).tolist(), np.asarray(w, dtype=np.float64).tolist()):
    hi = a * b
    terms += [hi, float(Fraction(a) * Fraction(b) - Fraction(hi))]      # (the remainder of a product is a double)
  return math.fsum(terms), float(np.abs(np.asarray(v, dtype=np.float64) * np.asarray(w, dtype=np.float64)).sum())
