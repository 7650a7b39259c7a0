"""The references of tests/step_kernels_ref.py checked on their own, without a GPU, so that the GPU tests do not rest on
an unchecked restatement: adjoints against central differences in float64, the component order against the centres of
oracle.losses, the uniform's range and granularity, the offset rule of philox_words, and Adam's first step."""
from fractions import Fraction

import numpy as np
import pytest

import step_kernels_ref as sk
from oracle import losses as ol

DRIFT_DIMS = [(None, 1), (None, 5), ("ou", 1), ("ou", 3), ("ou", 6), ("gradient", 2), ("nongradient", 2), ("lorenz", 3)]
RKL_SPECS = [(1.0, 10.0), (2.0, 1.0)]


def _central(f, x, h):
  """d f / d x by central differences, f scalar, x any shape"""
  g = np.empty_like(x)
  it = np.nditer(x, flags=["multi_index"])
  for _ in it:
    k = it.multi_index
    xp, xm = x.copy(), x.copy()
    xp[k] += h
    xm[k] -= h
    g[k] = (f(xp) - f(xm)) / (2 * h)
  return g


@pytest.mark.parametrize("drift,D", DRIFT_DIMS)
def test_score_residual_adjoints_equal_central_differences(oracle_lib, drift, D):
  n, count, dt, coef, a, c = 7, 3, 0.01, 0.7, 1.3, 0.37
  rng = np.random.default_rng(3 + D)
  r, score = 1.5 * rng.normal(size=(3 * n, D)), rng.normal(size=(n, D))
  sums, rbar, sbar = sk.score_residual_ref(r, score, n, count, D, dt, coef, drift, a, c)
  assert sums.shape == (3,) and rbar.shape == (3 * n, D) and sbar.shape == (n, D)
  u = sk.score_residual_u(r, score, n, D, dt, coef, drift, a)
  np.testing.assert_allclose(sums, [(u[:3] ** 2).sum(), (u[3:6] ** 2).sum(), (u[6:] ** 2).sum()], rtol=1e-14)
  loss = lambda rr, ss: c * sk.score_residual_ref(rr, ss, n, count, D, dt, coef, drift, a, c)[0].sum()
  # u is at most quadratic in r (cubic for the 2-D gradient field): the difference's own error is O(h^2) of the third
  # derivative, next to entries of size 2 c |u| / dt ~ 1e4
  fd_r = _central(lambda rr: loss(rr, score), r, 1e-5)
  fd_s = _central(lambda ss: loss(r, ss), score, 1e-5)
  scale = np.abs(rbar).max()
  assert np.abs(fd_r - rbar).max() <= 1e-8 * scale, np.abs(fd_r - rbar).max() / scale
  assert np.abs(fd_s - sbar).max() <= 1e-8 * scale
  if drift is not None:                                       # the r3 block is the drift's alone: it must not vanish
    assert np.abs(rbar[2 * n:]).min() > 0.0
    np.testing.assert_allclose(fd_r[2 * n:], rbar[2 * n:], rtol=1e-6, atol=1e-9 * scale)
  else:
    assert not rbar[2 * n:].any()


@pytest.mark.parametrize("D", [1, 2, 6, 10])
@pytest.mark.parametrize("T,beta", RKL_SPECS)
@pytest.mark.parametrize("tf", [0.0, 0.3, 1.0])
def test_rkl_residual_adjoints_equal_central_differences(D, T, beta, tf):
  t, c = tf * T, 0.37
  rng = np.random.default_rng(D)
  y = np.concatenate([1.5 * rng.normal(size=(9, D)), sk.rkl_far_rows(D).astype(np.float64)])
  lp = rng.normal(size=y.shape[0])
  total, ybar, lpbar = sk.rkl_residual_ref(y, lp, t, T, beta, c)
  logmix = sk.rkl_logmix(y, t, T, beta)[0]
  assert np.isfinite(logmix).all() and np.isfinite(ybar).all()        # the hand-placed rows included
  assert total == (lp - logmix).sum() and np.all(lpbar == c)
  fd = _central(lambda yy: c * sk.rkl_residual_ref(yy, lp, t, T, beta, c)[0], y, 1e-6)
  np.testing.assert_allclose(fd, ybar, rtol=1e-6, atol=1e-7)
  # against the reference's own loss: the mean of lp - log(mixture)
  src, tgt = ol._mvn_iso_pdf(y, 2.0 / beta * (T + 1.0)), ol._mvn_iso_pdf(y, 2.0 / beta)
  assert total == (lp - np.log(src * (T - t) / T + tgt * t / T)).sum()


def test_component_indexes_the_mixture_centres_in_the_kernels_order(oracle_lib):
  # mixture_source_kernel's cx / cy, times its R = 5
  cx = [0.0, 1.0, 0.0, -1.0, 0.6, 0.6, -0.6, -0.6]
  cy = [1.0, 0.0, -1.0, 0.0, 0.8, -0.8, -0.8, 0.8]
  np.testing.assert_allclose(ol.MIXTURE_CENTERS, 5.0 * np.stack([cx, cy], 1), rtol=0, atol=1e-15)
  comp = sk.component(0x123456789ABCDEF1, 0, 4096)
  assert comp.min() == 0 and comp.max() == 7 and np.bincount(comp, minlength=8).min() > 4096 / 8 * 0.7
  assert np.array_equal(comp, sk.philox_words(0x123456789ABCDEF1, 0, 4096, 2) >> 29)


def test_uniform24_range_granularity_and_word_offsets(oracle_lib):
  key = 0xC0FFEE1234567
  u = sk.uniform24(key, 0, 5000)
  assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
  assert u.min() < 0.01 and u.max() > 0.99 and abs(u.mean() - 0.5) < 0.02
  for s in (0, 1, 2):
    whole = sk.philox_words(key, 0, 40, s)
    assert np.array_equal(sk.philox_words(key, 5, 7, s), whole[5:12])
    assert np.array_equal(sk.philox_words(key, 4, 4, s), whole[4:8])
  assert not np.array_equal(sk.philox_words(key, 0, 40, 1), sk.philox_words(key, 0, 40, 2))
  assert not np.array_equal(sk.philox_words(key, 0, 40, 1), sk.philox_words(key + 1, 0, 40, 1))
  # the block index's high word is counter word 1: elements past 2^34 are not those 2^34 before
  hi = sk.philox_words(key, 2 ** 34 - 3, 8, 1)
  assert not np.array_equal(hi[3:], sk.philox_words(key, 0, 5, 1))
  # stream 0 is the normal stream: word pair (e & 3) >> 1 of block e >> 2 through Box-Muller (cnf_oracle_normal_f64)
  w = sk.philox_words(key, 0, 8, 0).astype(np.float64)
  u1, u2 = (np.floor(w[0::2] / 256) + 1) * 2.0 ** -24, np.floor(w[1::2] / 256) * 2.0 ** -24
  rad = np.sqrt(-2.0 * np.log(u1))
  z = np.stack([rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)], 1).reshape(-1)
  np.testing.assert_allclose(oracle_lib.normal(key, 0, 8), z, rtol=0, atol=1e-12)


def test_adam_ref_first_step_moves_by_lr_sign_g():
  rng = np.random.default_rng(0)
  g = rng.normal(size=50)
  g = np.concatenate([g + 0.05 * np.sign(g), [0.0, 0.0]]).astype(np.float32)      # |g| >= 0.05: eps / |g| <= 2e-7
  p = rng.normal(size=g.size).astype(np.float32)
  zero = np.zeros_like(p)
  lr, eps = 1e-3, 1e-8
  p1, m, v = sk.adam_ref(p, g, zero, zero, lr, 0.9, 0.999, eps, 1)
  step = p1 - p.astype(np.float64)
  np.testing.assert_allclose(step[:50], -float(np.float32(lr)) * np.sign(g[:50]), rtol=1e-6)
  assert np.array_equal(p1[g == 0], p[g == 0].astype(np.float64)) and (g == 0).sum() == 2
  b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
  np.testing.assert_allclose(m, (1 - b1) * g.astype(np.float64), rtol=1e-15)
  np.testing.assert_allclose(v, (1 - b2) * g.astype(np.float64) ** 2, rtol=1e-15)
  # eps is outside the square root: at |g| = eps the first step is lr / 2, not lr / sqrt(2)
  pe, _, _ = sk.adam_ref([0.0], [1e-8], [0.0], [0.0], lr, 0.9, 0.999, eps, 1)
  assert abs(pe[0] / -float(np.float32(lr)) - 0.5) < 1e-6


def test_weighted_sum_ref_is_exact():
  v, w = np.array([1e16, 1.0, -1e16, 3.0]), np.array([1.0, 0.1, 1.0, 1.0 / 3.0])
  total, mag = sk.weighted_sum_ref(v, w)
  # (naive summation loses the small terms: 0.0; the exact sum is fl(0.1) + 3 fl(1/3), below 1.1 by more than half an ulp)
  assert total == float(Fraction(0.1) + 3 * Fraction(1.0 / 3.0)) == 1.0999999999999999 and mag == 2e16 + 1.1
  assert sk.weighted_sum_ref([], []) == (0.0, 0.0)
