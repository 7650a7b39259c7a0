"""GPU tests of the training step's model-free kernels through the C ABI, each against the float64 restatement of
tests/step_kernels_ref.py (checked on its own in test_step_kernels_ref_cpu.py) or bit for bit against the oracle's
Philox words: cnf_score_residual, cnf_rkl_residual, cnf_adam_step / cnf_adam_step_dev / cnf_step_begin,
cnf_weighted_sum, cnf_fill_uniform_dev, cnf_mixture_source_dev, cnf_fill_normal / cnf_fill_normal_dev and the grid wrap
of cnf_fill_normal_threefry.

Every tolerance is exact, taken from an existing test (named where used), or a float32 rounding bound derived in the
docstring of its test from the operation count, with EPS = 2^-24 the relative error of one float32 rounding.
Hyper-parameters reach the kernels as float32; the references take those float32 values widened.  Every output buffer
sits between sentinel words that must survive the call."""
import math

import numpy as np
import pytest
import torch

import oracle
import step_kernels_ref as sk
from oracle import losses as ol

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
SENTINEL = {torch.float32: 7.25, torch.float64: 7.25, torch.int32: 77, torch.int64: 77}
KEY = 0x123456789ABCDEF1


def f32(v):
  """the float32 value of a hyper-parameter, widened"""
  return float(np.float32(v))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def capi():
  from cnf_ot_amd import _capi
  _capi.lib()
  return _capi


def guarded(n, dtype, dev, pad=4):
  """(buffer, view of n elements `pad` elements in): all sentinel; pad = 4 floats keeps the view 16-byte aligned"""
  buf = torch.full((n + 2 * pad,), SENTINEL[dtype], dtype=dtype, device=dev)
  return buf, buf[pad:pad + n]


def intact(buf, n, pad=4):
  s = SENTINEL[buf.dtype]
  return bool((buf[:pad] == s).all()) and bool((buf[pad + n:] == s).all())


def untouched(buf):
  return bool((buf == SENTINEL[buf.dtype]).all())


def dstate(dev, step, key=KEY):
  """The step's device state { step count, key } as int64 words (the key's bits)"""
  words = np.array([step, key], dtype=np.uint64).view(np.int64)
  return torch.from_numpy(words.copy()).to(dev)


# =====================================================================================================================
# cnf_score_residual
# =====================================================================================================================
SCORE_DRIFTS = [(1, None), (2, None), (2, "ou"), (2, "gradient"), (2, "nongradient"), (3, "lorenz"), (3, "ou"), (6, "ou"),
                (14, None)]
# slices that end at a wave's edge (64), one lane past it (65), inside a wave (63, 1000), inside the last partial wave
# (4099 = 63 * 65 + 4; 777 < count), one sample per slice, and several workgroups per slice
SCORE_SHAPES = [(1, 1), (1000, 1), (1000, 63), (4096, 64), (4099, 65), (777, 1000), (65537, 4096)]
DT, COEF, DRIFT_A, LOSS_COEF = 0.01, 0.7, 1.3, 0.37


def _drift_magnitudes(drift, r3, a):
  """(M [n, D], MJ [n, D, D]): the sums of the absolute monomials of drift_d and of d drift_d / d r_e -- what one
  float32 rounding inside their evaluation is relative to"""
  n, D = r3.shape
  M, MJ = np.zeros((n, D)), np.zeros((n, D, D))
  if drift == "ou":
    M = a * np.abs(r3)
    MJ[:, np.arange(D), np.arange(D)] = a
  elif drift == "gradient":
    x, y = np.abs(r3[:, 0]), np.abs(r3[:, 1])
    q = x * x + y * y + 4.0
    M[:, 0], M[:, 1] = a * q * x, a * (q * y + 2 * y + 2)
    MJ[:, 0, 0], MJ[:, 1, 1] = a * (q + 2 * x * x), a * (q + 2 * y * y + 2)
    MJ[:, 0, 1] = MJ[:, 1, 0] = a * 2 * x * y
  elif drift == "nongradient":
    x, y = np.abs(r3[:, 0]), np.abs(r3[:, 1])
    M[:, 0], M[:, 1] = a * x + 0.5 * y, a * y + 0.5 * x
    MJ[:, 0, 0] = MJ[:, 1, 1] = a
    MJ[:, 0, 1] = MJ[:, 1, 0] = 0.5
  elif drift == "lorenz":
    x, y, z = np.abs(r3[:, 0]), np.abs(r3[:, 1]), np.abs(r3[:, 2])
    M[:, 0], M[:, 1], M[:, 2] = 10 * (x + y), 28 * x + 9 * x * z + y, 9 * x * y + 8 * z / 3
    MJ[:, 0, 0] = MJ[:, 0, 1] = 10.0
    MJ[:, 1, 0], MJ[:, 1, 1], MJ[:, 1, 2] = 28 + 9 * z, 1.0, 9 * x
    MJ[:, 2, 0], MJ[:, 2, 1], MJ[:, 2, 2] = 9 * y, 9 * x, 8.0 / 3.0
  return M, MJ


def _score_call(capi, dev, r, score, n, count, D, drift, adjoints, dt=DT):
  n_slices = -(-n // count)
  sbuf, sums = guarded(n_slices, torch.float64, dev)
  rbuf, rbar = guarded(3 * n * D, torch.float32, dev)
  cbuf, sbar = guarded(n * D, torch.float32, dev)
  rc = capi.lib().cnf_score_residual(r.data_ptr(), score.data_ptr(), n, count, D, dt, COEF, sk.DRIFT_CODES[drift], DRIFT_A,
                                     LOSS_COEF, sums.data_ptr(), rbar.data_ptr() if adjoints else None,
                                     sbar.data_ptr() if adjoints else None, None)
  torch.cuda.synchronize()
  assert rc == capi.CNF_OK, rc
  assert intact(sbuf, n_slices) and intact(rbuf, 3 * n * D) and intact(cbuf, n * D)
  if not adjoints:
    assert untouched(rbuf) and untouched(cbuf)
  return sums.cpu().numpy(), rbar.cpu().numpy().reshape(3 * n, D), sbar.cpu().numpy().reshape(n, D)


@pytest.mark.parametrize("n,count", SCORE_SHAPES)
@pytest.mark.parametrize("D,drift", SCORE_DRIFTS)
def test_score_residual_sums_and_adjoints(dev, capi, D, drift, n, count):
  """cnf_score_residual against score_residual_ref, with and without adjoints.

  Sums: the rule of test_gpu_grad.py::test_term_residual_sums_and_adjoints.check -- rtol 2e-6, atol 2e-6 max|want| /
  min(count, 100).

  Adjoints, per entry.  Let T_d = |r2 - r1| / dt + |coef score_d| + M_d, M_d the sum of the absolute monomials of
  drift_d: the size of the terms u_d is made of.  The kernel rounds r2 - r1 (1), 1 / dt (1), their product (1), the
  fma with coef score (1), the drift (up to 7 roundings of its monomials: the 2-D gradient field) and the subtraction
  (1): |du_d| <= 8 EPS T_d.  u_bar = 2 c u adds one rounding, the product with 1 / dt two more (the quotient's own and
  the product's), with coef or a one:  |d rbar_{1,2}| <= 11 EPS (2 c / dt) T_d,  |d sbar| <= 11 EPS 2 c coef T_d, and for
  the OU drift |d rbar_3| <= 11 EPS 2 c a T_d.  The coupled fields' rbar_3,e = -sum_d u_bar_d J_de carries u_bar's 9 EPS
  T_d, up to 5 roundings inside J_de relative to its absolute monomials MJ_de, the product and the sum:
  |d rbar_3,e| <= 19 EPS 2 c sum_d T_d MJ_de.  Without a drift rbar_3 is exactly zero.  These are bounds relative to
  an entry's TERMS (about 1e-6 of them), not to its cancelled value."""
  rng = np.random.default_rng(1000 * D + n + count)
  r = (1.5 * rng.normal(size=(3 * n, D))).astype(np.float32)
  score = rng.normal(size=(n, D)).astype(np.float32)
  dt, coef, a, c = f32(DT), f32(COEF), f32(DRIFT_A), f32(LOSS_COEF)
  want_sums, want_rbar, want_sbar = sk.score_residual_ref(r, score, n, count, D, dt, coef, drift, a, c)
  rd, sd = torch.from_numpy(r).to(dev), torch.from_numpy(score).to(dev)

  sums0, _, _ = _score_call(capi, dev, rd, sd, n, count, D, drift, adjoints=False)
  sums1, rbar, sbar = _score_call(capi, dev, rd, sd, n, count, D, drift, adjoints=True)
  atol = 2e-6 * np.abs(want_sums).max() / min(count, 100)
  for name, sums in (("value", sums0), ("value+adjoints", sums1)):
    err = np.abs(sums - want_sums)
    print(f"[score_residual D={D} {drift} n={n} count={count} {name}] sums worst err / (atol + rtol |want|) "
          f"{(err / (atol + 2e-6 * np.abs(want_sums))).max():.3f}")
    assert (err <= atol + 2e-6 * np.abs(want_sums)).all()

  r64 = r.astype(np.float64)
  M, MJ = _drift_magnitudes(drift, r64[2 * n:], a)
  T = np.abs(r64[n:2 * n] - r64[:n]) / dt + np.abs(coef * score.astype(np.float64)) + M
  b12 = 11 * EPS * (2 * c / dt) * T
  if drift is None:
    b3 = np.zeros_like(T)
  elif drift == "ou":
    b3 = 11 * EPS * 2 * c * a * T
  else:
    b3 = 19 * EPS * 2 * c * np.einsum("id,ide->ie", T, MJ)
  bound_r = np.concatenate([b12, b12, b3])
  bound_s = 11 * EPS * 2 * c * coef * T
  er, es = np.abs(rbar - want_rbar), np.abs(sbar - want_sbar)
  worst3 = (er[2 * n:] / b3).max() if drift is not None else 0.0
  print(f"[score_residual D={D} {drift} n={n} count={count}] worst err / bound: rbar12 {(er[:2 * n] / bound_r[:2 * n]).max():.3f} "
        f"rbar3 {worst3:.3f} sbar {(es / bound_s).max():.3f}   max |rbar| {np.abs(want_rbar).max():.3g}")
  assert np.isfinite(rbar).all() and np.isfinite(sbar).all()
  assert (er <= bound_r).all() and (es <= bound_s).all()
  if drift is None:
    assert not rbar[2 * n:].any()


def test_score_residual_rejects_invalid_calls(dev, capi):
  n, count = 100, 10
  r = torch.randn(3 * n, 3, device=dev)
  score = torch.randn(n, 3, device=dev)
  sums = torch.full((n,), 7.25, dtype=torch.float64, device=dev)
  rbar, sbar = torch.full((3 * n * 3,), 7.25, device=dev), torch.full((n * 3,), 7.25, device=dev)
  lib = capi.lib()

  def call(D=2, drift="ou", count=count, dt=DT, rb=rbar.data_ptr(), sb=sbar.data_ptr()):
    return lib.cnf_score_residual(r.data_ptr(), score.data_ptr(), n, count, D, dt, COEF, sk.DRIFT_CODES[drift], DRIFT_A,
                                  LOSS_COEF, sums.data_ptr(), rb, sb, None)

  bad = [call(sb=None), call(rb=None), call(D=3, drift="gradient"), call(D=3, drift="nongradient"), call(D=2, drift="lorenz"),
         call(count=0), call(dt=0.0)]
  torch.cuda.synchronize()
  assert bad == [capi.CNF_ERR_INVALID] * len(bad), bad
  assert untouched(sums) and untouched(rbar) and untouched(sbar)
  assert call() == capi.CNF_OK                      # the same call with nothing wrong runs
  torch.cuda.synchronize()
  assert not untouched(sums[:n // count]) and untouched(sums[n // count:])


# =====================================================================================================================
# cnf_rkl_residual
# =====================================================================================================================
RKL_SPECS = [(1.0, 10.0), (2.0, 1.0)]
RKL_N = [1, 63, 64, 257, 262144 + 77]        # the last: a second trip of the 1024 x 256 grid-stride loop


def _rkl_call(capi, dev, y, lp, n, D, t, T, beta, adjoints=True):
  obuf, out = guarded(1, torch.float64, dev)
  ybuf, ybar = guarded(n * D, torch.float32, dev)
  lbuf, lpbar = guarded(n, torch.float32, dev)
  rc = capi.lib().cnf_rkl_residual(y.data_ptr(), lp.data_ptr(), n, D, t, T, beta, LOSS_COEF, out.data_ptr(),
                                   ybar.data_ptr() if adjoints else None, lpbar.data_ptr() if adjoints else None, None)
  torch.cuda.synchronize()
  assert rc == capi.CNF_OK, rc
  assert intact(obuf, 1) and intact(ybuf, n * D) and intact(lbuf, n)
  if not adjoints:
    assert untouched(ybuf) and untouched(lbuf)
  return float(out.cpu()[0]), ybar.cpu().numpy().reshape(n, D), lpbar.cpu().numpy()


def _rkl_check(capi, dev, y, lp, D, t, T, beta, tag):
  """Sum: rtol 2e-6 of sum |lp_i - logmix_i|.  The kernel's roundings are relative to |lp_i| and |logmix_i|, so the inputs
  keep the two from cancelling: lp > 0, and logmix < 0 for both specs (2 pi v > 1 for either variance, so neither density
  reaches 1) -- asserted -- which makes sum |lp_i - logmix_i| = sum |lp_i| + |logmix_i|.  ybar = c g y with g = (ps / vs + pt / vt) / (ps + pt) in [1 / vs, 1 / vt],
  ps, pt the weighted densities.  The kernel makes them from float32 exponents e = -|y|^2 / (2 v) + l + log w; the
  rounding of e is absolute: D roundings for |y|^2, 2 for v, 2 for the product and quotient, 3 for l = -D/2 log(2 pi v),
  1 for the sum: |de| <= (D + 8) EPS (|y|^2 / (2 v) + |l| + |log w|) =: d_s, d_t, and exp adds 2 EPS each.  g moves
  with the exponents' difference by at most (1 / vt - 1 / vs) / 4 per unit (p (1 - p) <= 1/4), relative to g >= 1 / vs:
  T / 4.  With the quotient, sums and two products:  |d ybar| <= |ybar| ((T / 4) (d_s + d_t + 4 EPS) + 8 EPS).
  A zero weight takes its component (and its d) out.  lpbar == loss_coef exactly."""
  n = y.shape[0]
  Tf, bf, tf, c = f32(T), f32(beta), f32(t), f32(LOSS_COEF)
  want_sum, want_ybar, _ = sk.rkl_residual_ref(y, lp, tf, Tf, bf, c)
  logmix = sk.rkl_logmix(y, tf, Tf, bf)[0]
  assert np.isfinite(logmix).all() and np.isfinite(want_ybar).all(), "the float64 reference must be finite on every row"
  assert (logmix < 0).all() and (lp > 0).all()
  yd, lpd = torch.from_numpy(y).to(dev), torch.from_numpy(lp).to(dev)
  got0, _, _ = _rkl_call(capi, dev, yd, lpd, n, D, t, T, beta, adjoints=False)
  got1, ybar, lpbar = _rkl_call(capi, dev, yd, lpd, n, D, t, T, beta)
  scale = np.abs(lp.astype(np.float64) - logmix).sum()
  s2 = (y.astype(np.float64) ** 2).sum(1)
  d = np.zeros(n)
  for v, w in ((2.0 / bf * (Tf + 1.0), (Tf - tf) / Tf), (2.0 / bf, tf / Tf)):
    if w > 0:
      d += (D + 8) * EPS * (s2 / (2 * v) + abs(0.5 * D * math.log(2 * math.pi * v)) + abs(math.log(w)))
  bound = np.abs(want_ybar) * ((Tf / 4) * (d + 4 * EPS) + 8 * EPS)[:, None]
  err = np.abs(ybar - want_ybar)
  with np.errstate(invalid="ignore", divide="ignore"):
    ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
  print(f"[rkl_residual {tag} D={D} n={n} T={T} beta={beta} t={t}] sum {got1:.9g} want {want_sum:.9g} "
        f"rel to sum|term| {abs(got1 - want_sum) / scale:.2e} (2e-6)  ybar worst err / bound {np.nanmax(ratio):.3f}")
  assert math.isfinite(got0) and math.isfinite(got1) and np.isfinite(ybar).all(), "finite wherever the reference is"
  assert abs(got0 - want_sum) <= 2e-6 * scale and abs(got1 - want_sum) <= 2e-6 * scale
  assert (err <= bound).all()
  assert np.array_equal(lpbar, np.full(n, np.float32(LOSS_COEF)))


def _rkl_inputs(n, D, far):
  rng = np.random.default_rng(77 * D + n)
  y = (1.5 * rng.normal(size=(n, D))).astype(np.float32)
  if far:
    rows = sk.rkl_far_rows(D)
    y[:rows.shape[0]] = rows
  return y, (0.5 + np.abs(rng.normal(size=n))).astype(np.float32)      # lp > 0: see _rkl_check


@pytest.mark.parametrize("tf", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("T,beta", RKL_SPECS)
@pytest.mark.parametrize("n", RKL_N)
@pytest.mark.parametrize("D", [1, 2, 6, 10])
def test_rkl_residual_sum_and_adjoints(dev, capi, D, n, T, beta, tf):
  """cnf_rkl_residual against rkl_residual_ref (bounds: _rkl_check); from n = 63 the first six rows are the hand-placed
  ones of rkl_far_rows, out to |y_d| = 9.5"""
  y, lp = _rkl_inputs(n, D, far=n >= 63)
  _rkl_check(capi, dev, y, lp, D, tf * T, T, beta, "far+random" if n >= 63 else "random")


@pytest.mark.parametrize("tf", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("T,beta", RKL_SPECS)
@pytest.mark.parametrize("D", [1, 2, 6, 10])
def test_rkl_residual_far_rows_alone(dev, capi, D, T, beta, tf):
  """The hand-placed rows on their own.  At t == T the source's weight is zero; for these rows its exponent is the
  larger one and the target's lies more than float32's exponent range below it: a maximum taken over the unweighted
  exponents leaves log(0) (the float64 reference, linear in the densities, is finite)."""
  y = sk.rkl_far_rows(D)
  lp = np.linspace(0.5, 3.0, y.shape[0]).astype(np.float32)
  _rkl_check(capi, dev, y, lp, D, tf * T, T, beta, "far")


def test_rkl_residual_rejects_invalid_calls(dev, capi):
  y, lp = torch.randn(10, 2, device=dev), torch.randn(10, device=dev)
  out = torch.full((1,), 7.25, dtype=torch.float64, device=dev)
  ybar, lpbar = torch.full((20,), 7.25, device=dev), torch.full((10,), 7.25, device=dev)
  f = capi.lib().cnf_rkl_residual
  p = (y.data_ptr(), lp.data_ptr())
  bad = [f(*p, 10, 2, 0.5, 1.0, 10.0, 0.37, out.data_ptr(), ybar.data_ptr(), None, None),
         f(*p, 10, 2, 0.5, 1.0, 10.0, 0.37, out.data_ptr(), None, lpbar.data_ptr(), None),
         f(*p, 10, 0, 0.5, 1.0, 10.0, 0.37, out.data_ptr(), None, None, None),
         f(*p, 10, 2, 0.5, 0.0, 10.0, 0.37, out.data_ptr(), None, None, None),
         f(*p, 10, 2, 0.5, 1.0, 0.0, 0.37, out.data_ptr(), None, None, None),
         f(*p, -1, 2, 0.5, 1.0, 10.0, 0.37, out.data_ptr(), None, None, None)]
  torch.cuda.synchronize()
  assert bad == [capi.CNF_ERR_INVALID] * len(bad), bad
  assert untouched(out) and untouched(ybar) and untouched(lpbar)


# =====================================================================================================================
# cnf_adam_step, cnf_adam_step_dev, cnf_step_begin
# =====================================================================================================================
ADAM_N = [1, 255, 256, 257, 11824]
ADAM_STEPS = [1, 2, 3, 1000, 100000]
ADAM_HYPER = [(1e-3, 0.9, 0.999), (1e-3, 0.5, 0.9)]
ADAM_EPS = 1e-8


def _adam_inputs(n, fresh, seed):
  """Three gradient bands by element index: |g| ~ 1; |g| in [1e-12, 1e-7], with moments of that scale, so that
  sqrt(nu) ties with or falls below eps = 1e-8; exact zeros, every second of them with zero moments too."""
  rng = np.random.default_rng(seed)
  band = (np.arange(n) + seed) % 3
  small = lambda: 10.0 ** rng.uniform(-12, -7, n) * rng.choice([-1.0, 1.0], n)
  g = np.where(band == 0, rng.normal(size=n), np.where(band == 1, small(), 0.0))
  mu = np.where(band == 1, small(), 0.3 * rng.normal(size=n))
  nu = np.where(band == 1, small() ** 2, 0.1 * rng.normal(size=n) ** 2)
  still = (band == 2) & ((np.arange(n) // 3) % 2 == 0)
  mu[still], nu[still] = 0.0, 0.0
  if fresh:
    mu[:], nu[:] = 0.0, 0.0
  p = rng.normal(size=n)
  return tuple(v.astype(np.float32) for v in (p, g, mu, nu))


def _adam_check(capi, dev, n, step, lr, b1, b2, device_count, fresh=False):
  """Bounds: the float32 rounding bounds of step_kernels_ref.adam_bounds, derived in its docstring (shared with
  test_gpu_captured_step.py)."""
  lib = capi.lib()
  p, g, mu, nu = _adam_inputs(n, fresh, seed=n + step)
  (want_p, want_mu, want_nu), (bound_p, bound_mu, bound_nu), (rho1, rho2) = sk.adam_bounds(p, g, mu, nu, lr, b1, b2,
                                                                                         ADAM_EPS, step)
  bufs = [guarded(n, torch.float32, dev) for _ in range(4)]
  for (_, view), src in zip(bufs, (p, g, mu, nu)):
    view.copy_(torch.from_numpy(src))
  ptrs = [view.data_ptr() for _, view in bufs]
  if device_count:
    # the count reaches `step` by that many cnf_step_begin calls where that is quick, else by one from step - 1
    st = dstate(dev, 0 if step <= 3 else step - 1)
    for k in range(step if step <= 3 else 1):
      before = st.cpu().numpy().copy()
      assert lib.cnf_step_begin(st.data_ptr(), None) == capi.CNF_OK
      torch.cuda.synchronize()
      after = st.cpu().numpy()
      assert after[0] == before[0] + 1 and after[1] == before[1] == np.uint64(KEY).view(np.int64)
    assert int(st.cpu()[0]) == step
    rc = lib.cnf_adam_step_dev(*ptrs, n, lr, b1, b2, ADAM_EPS, st.data_ptr(), None)
  else:
    rc = lib.cnf_adam_step(*ptrs, n, lr, b1, b2, ADAM_EPS, step, None)
  torch.cuda.synchronize()
  assert rc == capi.CNF_OK, rc
  assert all(intact(buf, n) for buf, _ in bufs)
  got_p, got_g, got_mu, got_nu = (view.cpu().numpy() for _, view in bufs)
  assert np.array_equal(got_g, g)
  if device_count:
    assert np.array_equal(st.cpu().numpy(), dstate("cpu", step).numpy())          # the state is read, never written

  p64 = p.astype(np.float64)
  upd = np.abs(p64 - want_p)
  e_mu, e_nu, e_p = np.abs(got_mu - want_mu), np.abs(got_nu - want_nu), np.abs(got_p - want_p)
  worst = sk.worst_ratio

  upd_rel = float((np.abs((got_p.astype(np.float64) - p64) - (want_p - p64))[upd > 0] / upd[upd > 0]).max()) if (upd > 0).any() else 0.0
  print(f"[adam{'_dev' if device_count else ''} n={n} step={step} b=({b1}, {b2}){' fresh' if fresh else ''}] worst err / bound: "
        f"mu {worst(e_mu, bound_mu):.3f} nu {worst(e_nu, bound_nu):.3f} p {worst(e_p, bound_p):.3f}   "
        f"update off by {upd_rel:.2e} of itself at worst (rho1 {rho1:.1e} rho2 {rho2:.1e})")
  assert not (np.isnan(got_p).any() or np.isnan(got_mu).any() or np.isnan(got_nu).any())
  assert (e_mu <= bound_mu).all() and (e_nu <= bound_nu).all() and (e_p <= bound_p).all()
  still = (g == 0) & (mu == 0) & (nu == 0)
  assert np.array_equal(got_p[still].view(np.uint32), p[still].view(np.uint32))
  assert not got_mu[still].any() and not got_nu[still].any()
  assert n < 6 or still.any()


@pytest.mark.parametrize("device_count", [False, True])
@pytest.mark.parametrize("lr,b1,b2", ADAM_HYPER)
@pytest.mark.parametrize("step", ADAM_STEPS)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_moments_and_parameters(dev, capi, n, step, lr, b1, b2, device_count):
  """cnf_adam_step and cnf_adam_step_dev (its bias corrections from the device's step count) against adam_ref: both
  moments and the parameters, to the rounding bounds of _adam_check"""
  _adam_check(capi, dev, n, step, lr, b1, b2, device_count)


@pytest.mark.parametrize("device_count", [False, True])
@pytest.mark.parametrize("step", [1, 3])
def test_adam_from_a_fresh_start(dev, capi, step, device_count):
  """mu = nu = 0: the first step's update is lr g / (|g| + eps); where g = 0 nothing moves"""
  _adam_check(capi, dev, 257, step, 1e-3, 0.9, 0.999, device_count, fresh=True)


def test_adam_rejects_invalid_calls_and_n_zero_touches_nothing(dev, capi):
  lib = capi.lib()
  bufs = [torch.full((8,), 7.25, device=dev) for _ in range(4)]
  ptrs = [b.data_ptr() for b in bufs]
  st = dstate(dev, 5)
  hyper = (1e-3, 0.9, 0.999, ADAM_EPS)
  assert lib.cnf_adam_step(*ptrs, 8, *hyper, 0, None) == capi.CNF_ERR_INVALID
  assert lib.cnf_adam_step(*ptrs, -1, *hyper, 1, None) == capi.CNF_ERR_INVALID
  assert lib.cnf_adam_step_dev(*ptrs, -1, *hyper, st.data_ptr(), None) == capi.CNF_ERR_INVALID
  assert lib.cnf_adam_step_dev(*ptrs, 8, *hyper, None, None) == capi.CNF_ERR_INVALID
  assert lib.cnf_step_begin(None, None) == capi.CNF_ERR_INVALID
  assert lib.cnf_adam_step(*ptrs, 0, *hyper, 1, None) == capi.CNF_OK
  assert lib.cnf_adam_step_dev(*ptrs, 0, *hyper, st.data_ptr(), None) == capi.CNF_OK
  torch.cuda.synchronize()
  assert all(untouched(b) for b in bufs) and np.array_equal(st.cpu().numpy(), dstate("cpu", 5).numpy())


# =====================================================================================================================
# cnf_weighted_sum
# =====================================================================================================================
def _weighted_sum_check(capi, dev, v, w, tag):
  """|got - exact| <= n 2^-53 sum |v_i w_i|.  A rounding is at most 2^-53 of its result.  The products' roundings
  together are 2^-53 sum |v w|.  A thread adds ceil(n / 256) products, the first to zero (exact): over all threads each
  later addition rounds by no more than 2^-53 sum |v w| in total, and so does each of the tree's min(8, ceil(log2 n))
  levels that add two nonzero values.  1 + (ceil(n / 256) - 1) + min(8, ceil(log2 n)) <= n for every n >= 1."""
  n = len(v)
  lib = capi.lib()
  vd = torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dev) if n else torch.zeros(1, dtype=torch.float64, device=dev)
  wd = torch.from_numpy(np.asarray(w, dtype=np.float64)).to(dev) if n else torch.zeros(1, dtype=torch.float64, device=dev)
  got = []
  for _ in range(2):
    buf, out = guarded(1, torch.float64, dev)
    assert lib.cnf_weighted_sum(vd.data_ptr(), wd.data_ptr(), n, out.data_ptr(), None) == capi.CNF_OK
    torch.cuda.synchronize()
    assert intact(buf, 1)
    got.append(out.cpu().numpy().copy())
  assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))           # a fixed order: the same bits
  want, mag = sk.weighted_sum_ref(v, w)
  bound = n * 2.0 ** -53 * mag
  err = abs(float(got[0][0]) - want)
  print(f"[weighted_sum {tag} n={n}] got {float(got[0][0]):.17g} want {want:.17g} err {err:.3e} bound {bound:.3e} "
        f"(|sum| / sum|vw| {abs(want) / mag if mag else 0:.1e})")
  assert err <= bound
  return float(got[0][0])


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 70001])
def test_weighted_sum_against_the_exact_sum(dev, capi, n):
  rng = np.random.default_rng(n)
  v, w = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n), rng.normal(size=n)
  got = _weighted_sum_check(capi, dev, v, w, "random")
  if n == 0:
    assert got == 0.0 and math.copysign(1.0, got) == 1.0


def test_weighted_sum_that_cancels(dev, capi):
  """Mixed signs whose sum is about 1e-12 of sum |v w|: the bound is relative to the terms, not to the result"""
  n = 1000
  rng = np.random.default_rng(5)
  v, w = rng.normal(size=n), rng.normal(size=n)
  rest, mag = sk.weighted_sum_ref(v[:-1], w[:-1])
  w[-1] = (-rest + 1e-12 * mag) / v[-1]
  want, mag = sk.weighted_sum_ref(v, w)
  assert 1e-13 < abs(want) / mag < 1e-11
  _weighted_sum_check(capi, dev, v, w, "cancelling")


def test_weighted_sum_rejects_invalid_calls(dev, capi):
  lib = capi.lib()
  v = torch.ones(4, dtype=torch.float64, device=dev)
  out = torch.full((1,), 7.25, dtype=torch.float64, device=dev)
  assert lib.cnf_weighted_sum(v.data_ptr(), v.data_ptr(), -1, out.data_ptr(), None) == capi.CNF_ERR_INVALID
  assert lib.cnf_weighted_sum(None, v.data_ptr(), 4, out.data_ptr(), None) == capi.CNF_ERR_INVALID
  assert lib.cnf_weighted_sum(v.data_ptr(), v.data_ptr(), 4, None, None) == capi.CNF_ERR_INVALID
  torch.cuda.synchronize()
  assert untouched(out)


# =====================================================================================================================
# cnf_fill_uniform_dev, cnf_mixture_source_dev
# =====================================================================================================================
WRAP_4096 = 4096 * 256           # the grid of the uniform and mixture kernels


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("n", [1, 5, WRAP_4096 + 259])
@pytest.mark.parametrize("first", [0, 1, 2, 3, 2 ** 34 - 3])
def test_fill_uniform_dev_equals_the_philox_words(dev, capi, first, n, scale):
  """Bit for bit: float32(scale) * float32(the word's top 24 bits / 2^24) -- the quotient is exact, the product rounds
  once.  first = 2^34 - 3 crosses into a block index above 2^32 (counter word 1 = 1); the largest n wraps the grid."""
  st = dstate(dev, 9)
  buf, out = guarded(n, torch.float32, dev)
  rc = capi.lib().cnf_fill_uniform_dev(st.data_ptr(), first, n, scale, out.data_ptr(), None)
  torch.cuda.synchronize()
  assert rc == capi.CNF_OK and intact(buf, n)
  want = np.float32(scale) * sk.uniform24(KEY, first, n).astype(np.float32)
  got = out.cpu().numpy()
  wrong = int((got.view(np.uint32) != want.view(np.uint32)).sum())
  print(f"[fill_uniform first={first} n={n} scale={scale}] {wrong} of {n} words differ; range [{got.min():.3g}, {got.max():.3g}]")
  assert wrong == 0
  assert np.array_equal(st.cpu().numpy(), dstate("cpu", 9).numpy())


def _mixture_call(capi, dev, st, first, n, z, want_out, want_comp):
  obuf, out = guarded(2 * n, torch.float32, dev)
  cbuf, comp = guarded(n, torch.int32, dev)
  rc = capi.lib().cnf_mixture_source_dev(st.data_ptr(), first, n, None if z is None else z.data_ptr(),
                                         out.data_ptr() if want_out else None, comp.data_ptr() if want_comp else None, None)
  torch.cuda.synchronize()
  assert rc == capi.CNF_OK, rc
  assert intact(obuf, 2 * n) and intact(cbuf, n)
  if not want_out:
    assert untouched(obuf)
  if not want_comp:
    assert untouched(cbuf)
  return out.cpu().numpy().reshape(n, 2), comp.cpu().numpy()


@pytest.mark.parametrize("n", [1, 5, 1000, WRAP_4096 + 3])
def test_mixture_source_dev_components_and_points(dev, capi, n):
  """comp == the top 3 bits of the stream-2 word, exactly.  out = z + 5 centre[comp]: the centre's product rounds in
  float32 and the sum once more, or one fma rounds the sum of z and the exact product of 5 and the float32 centre;
  either way within one float32 ulp at the larger of |5 centre| and the result."""
  st = dstate(dev, 3)
  rng = np.random.default_rng(n)
  z = rng.normal(size=(n, 2)).astype(np.float32)
  zd = torch.from_numpy(z).to(dev)
  want_comp = sk.component(KEY, 0, n)
  out, comp = _mixture_call(capi, dev, st, 0, n, zd, True, True)
  assert np.array_equal(comp.astype(np.int64), want_comp)
  centre = ol.MIXTURE_CENTERS[want_comp]
  want = z.astype(np.float64) + centre
  ulp = np.spacing(np.maximum(np.abs(centre), np.abs(want)).astype(np.float32)).astype(np.float64)
  err = np.abs(out - want)
  print(f"[mixture_source n={n}] components {np.bincount(want_comp, minlength=8).tolist()}  worst |out - want| / ulp {(err / ulp).max():.3f}")
  assert (err <= ulp).all()
  only_comp = _mixture_call(capi, dev, st, 0, n, None, False, True)[1]
  only_out = _mixture_call(capi, dev, st, 0, n, zd, True, False)[0]
  assert np.array_equal(only_comp, comp) and np.array_equal(only_out.view(np.uint32), out.view(np.uint32))
  for k in (1, 2, 3, 5):          # a later first sample: the rows from k of the whole call
    if k < n:
      m = min(n - k, 300)
      o, c = _mixture_call(capi, dev, st, k, m, zd[k:k + m].contiguous(), True, True)
      assert np.array_equal(c, comp[k:k + m]) and np.array_equal(o.view(np.uint32), out[k:k + m].view(np.uint32))
  assert np.array_equal(st.cpu().numpy(), dstate("cpu", 3).numpy())


def test_mixture_source_dev_rejects_invalid_calls(dev, capi):
  st = dstate(dev, 3)
  out, comp = torch.full((16,), 7.25, device=dev), torch.full((8,), 77, dtype=torch.int32, device=dev)
  z = torch.zeros(16, device=dev)
  f = capi.lib().cnf_mixture_source_dev
  bad = [f(st.data_ptr(), 0, 8, None, out.data_ptr(), comp.data_ptr(), None),       # out without z
         f(st.data_ptr(), 0, 8, z.data_ptr(), None, None, None),                    # nothing to write
         f(None, 0, 8, z.data_ptr(), out.data_ptr(), comp.data_ptr(), None),
         f(st.data_ptr(), 0, -1, z.data_ptr(), out.data_ptr(), comp.data_ptr(), None)]
  torch.cuda.synchronize()
  assert bad == [capi.CNF_ERR_INVALID] * len(bad), bad
  assert untouched(out) and untouched(comp)


# =====================================================================================================================
# cnf_fill_normal, cnf_fill_normal_dev, cnf_fill_normal_threefry
# =====================================================================================================================
TOL_NORMAL = 2e-5                 # test_gpu_parity.py's bound of cnf_fill_normal against oracle.normal
WRAP_NORMAL = 8192 * 256 * 4      # elements of one trip of fill_normal_kernel's grid (one block of 4 per thread)
SEED = 0x0FEDCBA987654321


def _normal_pair(capi, dev, first, n, pad=4):
  """The seeded call and the device-keyed call with the same key: (seeded [n] on the device, identical bits asserted)"""
  lib = capi.lib()
  st = dstate(dev, 1, SEED)
  b0, a = guarded(n, torch.float32, dev, pad)
  b1, b = guarded(n, torch.float32, dev, pad)
  assert lib.cnf_fill_normal(SEED, first, n, a.data_ptr(), None) == capi.CNF_OK
  assert lib.cnf_fill_normal_dev(st.data_ptr(), first, n, b.data_ptr(), None) == capi.CNF_OK
  torch.cuda.synchronize()
  assert intact(b0, n, pad) and intact(b1, n, pad)
  assert torch.equal(a.view(torch.int32), b.view(torch.int32))
  return a


def test_fill_normal_across_the_grid_wrap(dev, capi):
  """One call of 8192 x 256 x 4 + 1027 elements: its start, the elements across the grid-stride wrap and its end against
  oracle.normal at the same offsets"""
  n = WRAP_NORMAL + 1027
  z = _normal_pair(capi, dev, 0, n)
  for name, lo in (("start", 0), ("wrap", WRAP_NORMAL - 3072), ("end", n - 4096)):
    got = z[lo:lo + 4096].cpu().numpy().astype(np.float64)
    err = np.abs(got - oracle.normal(SEED, lo, 4096)).max()
    print(f"[fill_normal n={n} {name} window at {lo}] max err {err:.2e} ({TOL_NORMAL})")
    assert err <= TOL_NORMAL
  assert bool(torch.isfinite(z).all())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("first", [0, 1, 2, 3, 1000, 1001, 1002, 1003])
def test_fill_normal_at_every_offset_in_a_block(dev, capi, first, n):
  """The two ends of the range: a first element anywhere in its block of four, lengths that end anywhere in theirs"""
  z = _normal_pair(capi, dev, first, n).cpu().numpy().astype(np.float64)
  assert np.abs(z - oracle.normal(SEED, first, n)).max() <= TOL_NORMAL


@pytest.mark.parametrize("first", [0, 2])
def test_fill_normal_into_an_unaligned_output(dev, capi, first):
  """An output one float past a 16-byte boundary takes the scalar stores: the same bits as the aligned call"""
  n = 1000 + first
  aligned = _normal_pair(capi, dev, first, n, pad=4)
  shifted = _normal_pair(capi, dev, first, n, pad=5)
  assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
  assert torch.equal(aligned.view(torch.int32), shifted.view(torch.int32))
  assert np.abs(aligned.cpu().numpy().astype(np.float64) - oracle.normal(SEED, first, n)).max() <= TOL_NORMAL


def test_fill_normal_past_block_index_two_to_the_32(dev, capi):
  """first_element = 2^34 - 6, n = 12: the block index crosses 2^32, counter word 1 becomes 1"""
  first = 2 ** 34 - 6
  z = _normal_pair(capi, dev, first, 12).cpu().numpy().astype(np.float64)
  want = oracle.normal(SEED, first, 12)
  print(f"[fill_normal first=2^34-6] max err {np.abs(z - want).max():.2e}")
  assert np.abs(z - want).max() <= TOL_NORMAL
  assert np.abs(want[6:] - oracle.normal(SEED, 0, 6)).max() > 0.1          # not the stream's start again


def test_fill_normal_threefry_across_the_grid_wrap(dev, capi):
  """One call whose in-call index crosses the 8192 x 256 grid: a window across the wrap against
  oracle.normal_threefry, under the tolerances of test_gpu_parity.py::test_threefry_normals_match_oracle (float64
  1e-11: two erfinv implementations; float32 5e-7)"""
  wrap = 8192 * 256
  size = wrap + 600
  b64, out64 = guarded(size, torch.float64, dev)
  b32, out32 = guarded(size, torch.float32, dev)
  rc = capi.lib().cnf_fill_normal_threefry(7, 42, size, 0, size, out32.data_ptr(), out64.data_ptr(), None)
  torch.cuda.synchronize()
  assert rc == capi.CNF_OK and intact(b64, size) and intact(b32, size)
  lo, m = wrap - 600, 1200
  want = oracle.normal_threefry((7, 42), size, first_element=lo, n=m)
  e64 = np.abs(out64[lo:lo + m].cpu().numpy() - want).max()
  e32 = np.abs(out32[lo:lo + m].cpu().numpy().astype(np.float64) - want).max()
  print(f"[threefry size={size} window at {lo}] max err f64 {e64:.2e} (1e-11) f32 {e32:.2e} (5e-7)")
  assert e64 <= 1e-11 and e32 <= 5e-7
  assert bool(torch.isfinite(out64).all())
