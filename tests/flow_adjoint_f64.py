"""An analytic reverse-mode pass of the (non-periodized) flow in NumPy: the reference the backward kernels are held to,
tensor by tensor (test_gpu_flow_adjoint.py), itself checked against central differences of the C oracle over ALL
parameters (test_flow_adjoint_cpu.py).  Test helper: no tests here, no GPU, never imported from cnf_ot_amd/.

The forward follows oracle/numpy_flow.py (rqs_tables / rqs_forward / rqs_inverse and the composition of NumpyFlow),
with the bin picked by index instead of by mask; the backward is the transpose of those very statements, one
elementary operation at a time, in the order they were executed.  Nothing is taken from the kernels' own partials.
The code is generic in the dtype: the float64 run is the reference, the float32 run of the same statements is the
noise floor a float32 evaluation of the same algorithm has on a tensor (`e32`, see `bound`).  One run shows the
rounding of the knot positions only by luck: `knot_sensitivity` measures that part from the float64 pass.

A parameter gradient is discontinuous where a float32 evaluation can land on the other side of a ReLU (or, for the
log-det, of a knot).  `margins` measures how far a sample is from every such place; `select` removes the samples that
are too close BEFORE anything is compared (no exclusion by disagreement), and the share it may remove is capped."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np

import oracle
from step_kernels_ref import rkl_logmix, rkl_residual_ref, score_residual_ref, score_residual_u, slice_sums

KNOT_MARGIN, RELU_MARGIN, MAX_DROPPED = 1e-4, 1e-5, 0.05
# What a float32 knot carries at the least: one rounding in the widest binade of the splines' range, |x| in [8, 16)
# (half an ulp there).  See `knot_rounding`.
KNOT_ULP, KNOT_RUNS = 2.0 ** -21, 4
_knot_noise = None      # (size, numpy Generator) while a `knot_rounding` block runs
DRIFT_NAMES = {-1: None, 0: "ou", 1: "gradient", 2: "nongradient", 3: "lorenz"}
KINETIC, KINETIC_SCORE, FLOW_MATCHING, POTENTIAL, REVERSE_KL, NEG_LOGPROB = range(6)


def _cfg(cfg):
  """oracle.OracleConfig from it or from a cnf_ot_amd.FlowConfig"""
  if hasattr(cfg, "dim"):
    return oracle.OracleConfig(D=cfg.dim, L=cfg.num_layers, H=cfg.hidden_size, M=cfg.mlp_num_layers, K=cfg.num_bins,
                               range_min=cfg.range_min, range_max=cfg.range_max, min_bin_size=cfg.min_bin_size,
                               min_knot_slope=cfg.min_knot_slope)
  return cfg


def param_blocks(cfg):
  """[(name, offset, size)] of the flat layout, in the order and with the names of cnf_ot_amd.params.param_spec"""
  cfg = _cfg(cfg)
  P = 3 * cfg.K + 1
  out, off = [("~/first", 0, P)], P
  for l in range(cfg.L):
    for d in range(1, cfg.D):
      for m in range(cfg.M):
        rows = 1 + d if m == 0 else cfg.H
        out.append((f"mlp_layer{l}_d{d}/~/linear_{m}/w", off, rows * cfg.H)); off += rows * cfg.H
        out.append((f"mlp_layer{l}_d{d}/~/linear_{m}/b", off, cfg.H)); off += cfg.H
      out.append((f"linear_out_layer{l}_d{d}/w", off, cfg.H * P)); off += cfg.H * P
      out.append((f"linear_out_layer{l}_d{d}/b", off, P)); off += P
  return out


def expand_c(c, B, dt=np.float64):
  """[B] conditions: one value is broadcast, B values are per sample, S values are S slices of ceil(B / S) samples
  (the last may be short) -- NumpyFlow._c, and the C ABI's c[i / c_block]"""
  c = np.asarray(c, dtype=dt).reshape(-1)
  if c.size == 1:
    return np.full(B, c[0], dtype=dt)
  if c.size == B:
    return c
  block = -(-B // c.size)
  assert (B - 1) // block == c.size - 1, (B, c.size)
  return c[np.arange(B) // block]


class _Net:
  """the parameters as arrays of `dt`, and where each tensor's gradient goes"""

  def __init__(self, cfg, flat, dt):
    cfg = _cfg(cfg)
    assert not cfg.periodized
    self.cfg, self.dt = cfg, dt
    self.D, self.L, self.H, self.M, self.K = cfg.D, cfg.L, cfg.H, cfg.M, cfg.K
    self.P = 3 * cfg.K + 1
    flat = np.asarray(flat, dtype=dt).reshape(-1)
    self.n = flat.size
    self.first = flat[:self.P]
    self.cond = {}
    off = self.P
    for l in range(self.L):
      for d in range(1, self.D):
        lin = []
        for m in range(self.M + 1):
          rows = 1 + d if m == 0 else self.H
          cols = self.H if m < self.M else self.P
          lin.append((flat[off:off + rows * cols].reshape(rows, cols), flat[off + rows * cols:off + rows * cols + cols],
                      off, off + rows * cols))
          off += rows * cols + cols
        self.cond[(l, d)] = lin
    assert off == flat.size, (off, flat.size)
    a = lambda v: np.asarray(v, dtype=dt)
    self.lo, self.hi = a(cfg.range_min), a(cfg.range_max)
    self.min_bin, self.min_slope = a(cfg.min_bin_size), a(cfg.min_knot_slope)
    self.slope_offset = a(np.log(np.exp(1.0 - cfg.min_knot_slope) - 1.0))
    self.bin_scale = a((cfg.range_max - cfg.range_min) - cfg.K * cfg.min_bin_size)

  # ---- conditioner ----
  def theta(self, l, d, c, known):
    """(theta [B, P], record, per-sample ReLU margin)"""
    B = c.shape[0]
    if d == 0:
      return np.broadcast_to(self.first, (B, self.P)), None, np.full(B, np.inf)
    lin = self.cond[(l, d)]
    h = np.concatenate([c[:, None], known], axis=1)
    acts, pres, margin = [h], [], np.full(B, np.inf)
    for W, b, _, _ in lin[:-1]:
      pre = h @ W + b
      with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.minimum(margin, (np.abs(pre) / (np.abs(h) @ np.abs(W) + np.abs(b))).min(1).astype(np.float64))
      h = np.maximum(pre, 0)
      pres.append(pre); acts.append(h)
    W, b, _, _ = lin[-1]
    return h @ W + b, (acts, pres), margin

  def theta_bwd(self, l, d, rec, g, grad):
    """adds the parameter gradient of theta's adjoint g [B, P]; returns the adjoint of `known` [B, d] (None at d = 0)"""
    if d == 0:
      grad[:self.P] += g.sum(0)
      return None
    lin = self.cond[(l, d)]
    acts, pres = rec
    for m in range(self.M, -1, -1):
      W, _, ow, ob = lin[m]
      grad[ow:ob] += (acts[m].T @ g).ravel()
      grad[ob:ob + W.shape[1]] += g.sum(0)
      g = g @ W.T
      if m > 0:
        g = g * (pres[m - 1] > 0)
    return g[:, 1:]

  # ---- knot tables (numpy_flow.rqs_tables) ----
  def tables(self, theta):
    K = self.K
    B = theta.shape[0]

    def bins(u):
      e = np.exp(u - u.max(axis=1, keepdims=True))
      p = e / e.sum(axis=1, keepdims=True)
      w = p * self.bin_scale + self.min_bin
      lo, hi = np.full((B, 1), self.lo, dtype=self.dt), np.full((B, 1), self.hi, dtype=self.dt)
      return p, np.concatenate([lo, self.lo + np.cumsum(w[:, :-1], axis=1), hi], axis=1)

    pw, xk = bins(theta[:, :K])
    ph, yk = bins(theta[:, K:2 * K])
    if _knot_noise is not None:      # the interior knots moved by +- one float32 rounding each (the ends are constants)
      u, rng = _knot_noise
      for k in (xk, yk):
        k[:, 1:-1] += u * rng.choice([-1.0, 1.0], size=(B, K - 1))
    v = theta[:, 2 * K:] + self.slope_offset
    sp = np.logaddexp(v, np.zeros((), dtype=self.dt))
    return SimpleNamespace(xk=xk, yk=yk, dl=sp + self.min_slope, pw=pw, ph=ph, sig=np.exp(v - sp))

  def tables_bwd(self, tab, xkb, ykb, dlb):
    """theta's adjoint [B, P] from the tables' (the two end knots are constants)"""
    K = self.K

    def bins(p, kb):
      wb = np.zeros_like(p)
      wb[:, :K - 1] = np.cumsum(kb[:, 1:K][:, ::-1], axis=1)[:, ::-1]      # w_j enters every knot j + 1 .. K - 1
      return self.bin_scale * p * (wb - (p * wb).sum(axis=1, keepdims=True))

    return np.concatenate([bins(tab.pw, xkb), bins(tab.ph, ykb), dlb * tab.sig], axis=1)


def _spline(net, v, tab, inverse):
  """One rational-quadratic spline per row (numpy_flow.rqs_forward, inverse: rqs_inverse) with its linear tails:
  (result, log-det, record, knot margin)"""
  K = net.K
  ar = np.arange(v.shape[0])
  pos = tab.yk if inverse else tab.xk
  k = np.clip((v[:, None] >= pos[:, 1:-1]).sum(1), 0, K - 1)
  x0, x1, y0, y1, d0, d1 = tab.xk[ar, k], tab.xk[ar, k + 1], tab.yk[ar, k], tab.yk[ar, k + 1], tab.dl[ar, k], tab.dl[ar, k + 1]
  below, above = v <= pos[:, 0], v >= pos[:, -1]
  margin = (np.abs(v[:, None] - pos).min(1) / (pos[ar, k + 1] - pos[ar, k])).astype(np.float64)
  r = SimpleNamespace(k=k, v=v, inverse=inverse, below=below, above=above, x0=x0, y0=y0, d0=d0, d1=d1)
  r.bw, r.bh = x1 - x0, y1 - y0
  r.s = r.bh / r.bw
  r.st = d1 + d0 - 2 * r.s
  if not inverse:
    zr = (v - x0) / r.bw
    r.zin = (zr >= 0) & (zr <= 1)
    z = r.z = np.clip(zr, 0, 1)
  else:
    wr = (v - y0) / r.bh
    r.win = (wr >= 0) & (wr <= 1)
    w = r.w = np.clip(wr, 0, 1)
    r.c = -r.s * w
    r.b = d0 - r.st * w
    r.a = r.s - r.b
    r.r = np.sqrt(r.b * r.b - 4 * r.a * r.c)
    zr = -2 * r.c / (r.b + r.r)
    r.zin = (zr >= 0) & (zr <= 1)
    z = r.z = np.clip(zr, 0, 1)
  r.sqz, r.z1mz, r.sq1 = z * z, z - z * z, (1 - z) ** 2
  r.den = r.s + r.st * r.z1mz
  r.e = d1 * r.sqz + 2 * r.s * r.z1mz + d0 * r.sq1
  ld = 2 * np.log(r.s) + np.log(r.e) - 2 * np.log(r.den)
  dl0, dlK = tab.dl[:, 0], tab.dl[:, -1]
  if not inverse:
    r.num = r.s * r.sqz + d0 * r.z1mz
    r.q = r.num / r.den
    out = y0 + r.bh * r.q
    out = np.where(below, (v - tab.xk[:, 0]) * dl0 + tab.yk[:, 0], out)
    out = np.where(above, (v - tab.xk[:, -1]) * dlK + tab.yk[:, -1], out)
    ld = np.where(below, np.log(dl0), np.where(above, np.log(dlK), ld))
  else:
    out = r.bw * z + x0
    out = np.where(below, (v - tab.yk[:, 0]) / dl0 + tab.xk[:, 0], out)
    out = np.where(above, (v - tab.yk[:, -1]) / dlK + tab.xk[:, -1], out)
    ld = np.where(below, -np.log(dl0), np.where(above, -np.log(dlK), -ld))
  return out, ld, r, margin


def _spline_bwd(net, r, tab, ob, lb):
  """adjoints of (input [B], xk, yk, dl [B, K + 1]) from those of the result (ob) and the log-det (lb)"""
  inside = ~(r.below | r.above)
  ob_t, lb_t = ob, lb
  ob, lb = ob * inside, lb * inside
  s, st, z, d0, d1 = r.s, r.st, r.z, r.d0, r.d1
  if not r.inverse:
    y0b, bhb, qb = ob, ob * r.q, ob * r.bh
    numb = qb / r.den
    denb = -qb * r.q / r.den - 2 * lb / r.den
    eb, sb = lb / r.e, 2 * lb / s
    zb = 0
  else:
    zb, bwb, x0b = ob * r.bw, ob * z, ob
    eb, sb, denb = -lb / r.e, -2 * lb / s, 2 * lb / r.den
  # e = d1 z^2 + 2 s z(1-z) + d0 (1-z)^2;  den = s + st z(1-z)
  d1b, sqzb, z1mzb, d0b, sq1b = eb * r.sqz, eb * d1, eb * 2 * s, eb * r.sq1, eb * d0
  sb = sb + eb * 2 * r.z1mz + denb
  stb = denb * r.z1mz
  z1mzb = z1mzb + denb * st
  if not r.inverse:      # num = s z^2 + d0 z(1-z)
    sb = sb + numb * r.sqz
    sqzb = sqzb + numb * s
    d0b = d0b + numb * r.z1mz
    z1mzb = z1mzb + numb * d0
  zb = (zb + sqzb * 2 * z + z1mzb * (1 - 2 * z) - sq1b * 2 * (1 - z)) * r.zin
  if not r.inverse:      # z = (x - x0) / bw
    vb, x0b, bwb = zb / r.bw, -zb / r.bw, -zb * z / r.bw
  else:                  # z = -2 c / (b + r), r = sqrt(b^2 - 4 a c), a = s - b, b = d0 - st w, c = -s w, w = (y - y0) / bh
    t = r.b + r.r
    cb, tb = -2 * zb / t, -zb * z / t
    discb = tb / (2 * r.r)
    bb = tb + discb * 2 * r.b
    ab = -4 * discb * r.c
    cb = cb - 4 * discb * r.a
    sb = sb + ab
    bb = bb - ab
    d0b = d0b + bb
    stb = stb - bb * r.w
    wb = (-bb * st - cb * s) * r.win
    sb = sb - cb * r.w
    vb, y0b, bhb = wb / r.bh, -wb / r.bh, -wb * r.w / r.bh
  d1b, d0b, sb = d1b + stb, d0b + stb, sb - 2 * stb      # st = d1 + d0 - 2 s
  bhb = bhb + sb / r.bw                                 # s = bh / bw
  bwb = bwb - sb * s / r.bw
  B, ar, k = r.v.shape[0], np.arange(r.v.shape[0]), r.k
  xkb, ykb, dlb = (np.zeros((B, net.K + 1), dtype=net.dt) for _ in range(3))
  xkb[ar, k] += x0b - bwb; xkb[ar, k + 1] += bwb
  ykb[ar, k] += y0b - bhb; ykb[ar, k + 1] += bhb
  dlb[ar, k] += d0b; dlb[ar, k + 1] += d1b
  # the tails: result = (v - p_in) * slope + p_out (inverse: / slope), log-det = +- log slope; the end knots are constants
  for on, j in ((r.below, 0), (r.above, net.K)):
    dl = tab.dl[:, j]
    if not r.inverse:
      tv = ob_t * dl
      tdl = ob_t * (r.v - tab.xk[:, j]) + lb_t / dl
    else:
      tv = ob_t / dl
      tdl = -ob_t * (r.v - tab.yk[:, j]) / (dl * dl) - lb_t / dl
    vb = np.where(on, tv, vb)
    dlb[:, j] += np.where(on, tdl, 0)
  return vb, xkb, ykb, dlb


def _forward(net, pts, c, to_base):
  """NumpyFlow.inverse_logdet (to_base) / forward_logdet: (out, logdet, records, knot margin [B], ReLU margin [B])"""
  u = np.asarray(pts, dtype=net.dt)
  B, D = u.shape
  total = np.zeros(B, dtype=net.dt)
  knot, relu = np.full(B, np.inf), np.full(B, np.inf)
  recs = []
  for l in (reversed(range(net.L)) if to_base else range(net.L)):
    perm = np.arange(D) if l % 2 == 0 else np.arange(D)[::-1]
    out = np.zeros_like(u)
    per_d = []
    for d in range(D):
      i = perm[d]
      theta, crec, rm = net.theta(l, d, c, (out if to_base else u)[:, perm[:d]])
      tab = net.tables(theta)
      out[:, i], ld, srec, km = _spline(net, u[:, i], tab, inverse=not to_base)
      total = total + ld
      knot, relu = np.minimum(knot, km), np.minimum(relu, rm)
      per_d.append((crec, tab, srec))
    recs.append((l, perm, per_d))
    u = out
  return u, total, recs, knot, relu


def _backward(net, recs, ybar, ldbar, to_base, B):
  D = net.D
  ob = np.zeros((B, D), dtype=net.dt) if ybar is None else np.array(ybar, dtype=net.dt)
  lb = np.zeros(B, dtype=net.dt) if ldbar is None else np.asarray(ldbar, dtype=net.dt)
  grad = np.zeros(net.n, dtype=net.dt)
  for l, perm, per_d in reversed(recs):
    ub = np.zeros((B, D), dtype=net.dt)
    for d in (reversed(range(D)) if to_base else range(D)):
      i = perm[d]
      crec, tab, srec = per_d[d]
      vb, xkb, ykb, dlb = _spline_bwd(net, srec, tab, ob[:, i], lb)
      ub[:, i] += vb
      kb = net.theta_bwd(l, d, crec, net.tables_bwd(tab, xkb, ykb, dlb), grad)
      if d:      # the conditioner read this layer's outputs (to_base) / inputs
        (ob if to_base else ub)[:, perm[:d]] += kb
    ob = ub
  return ob, grad


@contextlib.contextmanager
def knot_rounding(seed, u=KNOT_ULP):
  """Inside the block every interior knot of every spline is moved by +-u (random signs): the float64 pass as it
  comes out when the knot positions are stored in float32."""
  global _knot_noise
  _knot_noise = (u, np.random.default_rng(seed))
  try:
    yield
  finally:
    _knot_noise = None


def _deviation(a, b):
  """elementwise |a - b| through tuples, lists and dicts of arrays (None stays None)"""
  if a is None:
    return None
  if isinstance(a, dict):
    return {k: _deviation(a[k], b[k]) for k in a}
  if isinstance(a, (tuple, list)):
    return tuple(_deviation(x, y) for x, y in zip(a, b))
  return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))


def _largest(a, b):
  if a is None:
    return None
  if isinstance(a, dict):
    return {k: _largest(a[k], b[k]) for k in a}
  if isinstance(a, tuple):
    return tuple(_largest(x, y) for x, y in zip(a, b))
  return np.maximum(a, b)


def knot_sensitivity(fn, base):
  """Elementwise, the largest change of fn()'s float64 results over KNOT_RUNS runs with the knots rounded
  (`knot_rounding`): the part of a float32 evaluation's error that ONE float32 run of this module shows only by luck.
  A point in a narrow, steep bin (bin height / width ~ 10) of a spline whose output feeds conditioners with |x| ~ 12
  turns 2^-21 in a knot into 1e-5 of the pass's value and 1e-3 of a first-layer weight's gradient; the float32 run
  here, the C oracle's float32 build and the kernels (either math mode) land anywhere in that range on such points."""
  dev = None
  for seed in range(KNOT_RUNS):
    with knot_rounding(seed):
      d = _deviation(fn(), base)
    dev = d if dev is None else _largest(dev, d)
  return dev


def pass_vjp(cfg, flat, pts, c, ybar, ldbar, to_base, dtype=np.float64):
  """(out [B, D], logdet [B], xbar [B, D], grad [n_params]) of one flow pass: to_base -> data -> base
  (NumpyFlow.inverse_logdet), else base -> data (forward_logdet); xbar and grad are the adjoints of the inputs and of
  the parameters for the output adjoints ybar [B, D] and ldbar [B] (None: zero)."""
  net = _Net(cfg, flat, dtype)
  pts = np.asarray(pts, dtype=dtype)
  B = pts.shape[0]
  out, ld, recs, _, _ = _forward(net, pts, expand_c(c, B, dtype), to_base)
  xbar, grad = _backward(net, recs, ybar, ldbar, to_base, B)
  return out, ld, xbar, grad


def margins(cfg, flat, pts, c, to_base):
  """per sample, from the float64 pass: (the smallest |spline input - knot| / bin width over all L D splines, the
  smallest |pre-activation| / (sum |w_i x_i| + |b|) over all ReLUs)"""
  net = _Net(cfg, flat, np.float64)
  pts = np.asarray(pts, dtype=np.float64)
  _, _, _, knot, relu = _forward(net, pts, expand_c(c, pts.shape[0]), to_base)
  return knot, relu


# ---- the loss terms --------------------------------------------------------------------------------------------------
def potential_grad(subtype, r, a):
  """grad V of oracle.losses.potential"""
  if subtype == 0:
    return r
  if subtype == 1:       # (|r - a 1| |r + a 1| / 2)^2
    m, p = r - a, r + a
    return ((m * (p * p).sum(1, keepdims=True)) + (p * (m * m).sum(1, keepdims=True))) / 2
  if subtype == 2:       # 50 exp(-|r|^2 / 2)
    return -50 * np.exp(-(r * r).sum(1, keepdims=True) / 2) * r
  raise ValueError(subtype)


def _potential(subtype, r, a):
  if subtype == 0:
    return (r * r).sum(1) / 2
  if subtype == 1:
    return ((r - a) ** 2).sum(1) * ((r + a) ** 2).sum(1) / 4
  return 50 * np.exp(-(r * r).sum(1) / 2)


def _term_slice(net, spec, z, ts):
  """one slice: (per-sample values [B], grad, knot margin [B], ReLU margin [B])"""
  dt_ = net.dt
  f = lambda v: np.asarray(v, dtype=dt_)
  B, D = z.shape
  k = spec.kind
  km, rm = np.full(B, np.inf), np.full(B, np.inf)

  def fwd(pts, c, to_base):
    nonlocal km, rm
    out, ld, recs, a, b = _forward(net, pts, np.full(pts.shape[0], c, dtype=dt_), to_base)
    km, rm = np.minimum(km, a), np.minimum(rm, b)
    return out, ld, recs

  def bwd(recs, yb, lb, to_base):
    return _backward(net, recs, yb, lb, to_base, B)

  ts = f(ts)
  if k == NEG_LOGPROB:
    x, ld, recs = fwd(z, ts, True)
    val = (x * x).sum(1) / 2 + f(0.5 * D * np.log(2 * np.pi)) - ld
    _, grad = bwd(recs, x, np.full(B, -1, dtype=dt_), True)
    return val, grad, km, rm
  if k == POTENTIAL:
    y, _, recs = fwd(z, ts, False)
    a = f(spec.a)
    _, grad = bwd(recs, potential_grad(spec.subtype, y, a), None, False)
    return _potential(spec.subtype, y, a), grad, km, rm
  if k == REVERSE_KL:
    y, ld, recs = fwd(z, ts, False)
    lp = -(z * z).sum(1) / 2 - f(0.5 * D * np.log(2 * np.pi)) - ld
    T, beta = float(spec.T), float(spec.beta)
    y64 = y.astype(np.float64)
    _, yb, lpb = rkl_residual_ref(y64, lp, float(ts), T, beta, 1.0)
    val = lp - f(rkl_logmix(y64, float(ts), T, beta)[0])
    _, grad = bwd(recs, f(yb), f(-lpb), False)
    return val, grad, km, rm
  h = f(spec.dt) / 2
  r1, _, rec1 = fwd(z, ts - h, False)
  r2, _, rec2 = fwd(z, ts + h, False)
  if k == KINETIC:
    v = (r2 - r1) / f(spec.dt)
    _, g1 = bwd(rec1, -2 * v / f(spec.dt), None, False)
    _, g2 = bwd(rec2, 2 * v / f(spec.dt), None, False)
    return (v * v).sum(1), g1 + g2, km, rm
  if k not in (KINETIC_SCORE, FLOW_MATCHING):
    raise ValueError(k)
  r3, _, rec3 = fwd(z, ts, False)
  dx = f(spec.dx)
  score, evals, a, b = _fd_score(net, r3, np.full(B, ts, dtype=dt_), dx)
  km, rm = np.minimum(km, a), np.minimum(rm, b)
  drift = DRIFT_NAMES[spec.subtype] if k == FLOW_MATCHING else None
  r = np.concatenate([r1, r2, r3]).astype(np.float64)
  _, rbar, sbar = score_residual_ref(r, score.astype(np.float64), B, B, D, float(spec.dt), float(spec.coef), drift,
                                     float(spec.a), 1.0)
  # the value from the very numbers of this dtype: u = (r2 - r1) / dt + coef score - drift(r3)
  u = score_residual_u(r, score.astype(np.float64), B, D, float(spec.dt), float(spec.coef), drift, float(spec.a))
  rbar = f(rbar)
  r3b, grad = _fd_score_bwd(net, evals, f(sbar), dx)
  r3b += rbar[2 * B:]
  for recs, rb in ((rec1, rbar[:B]), (rec2, rbar[B:2 * B]), (rec3, r3b)):
    grad += bwd(recs, rb, None, False)[1]
  return f((u * u).sum(1)), grad, km, rm


def _fd_score(net, r3, c, dx):
  """score[i, d] = (log_prob(r3_i + dx/2 e_d) - log_prob(r3_i - dx/2 e_d)) / dx (applications.py:264-273): (score, the
  2 D passes' records, knot margin, ReLU margin)"""
  B, D = r3.shape
  score = np.zeros((B, D), dtype=net.dt)
  evals, km, rm = [], np.full(B, np.inf), np.full(B, np.inf)
  for d in range(D):
    lps = []
    for sgn in (1, -1):
      p = r3.copy()
      p[:, d] += sgn * dx / 2
      x, ld, recs, a, b = _forward(net, p, c, True)
      km, rm = np.minimum(km, a), np.minimum(rm, b)
      lps.append(-(x * x).sum(1) / 2 + ld)
      evals.append((d, sgn, x, recs))
    score[:, d] = (lps[0] - lps[1]) / dx
  return score, evals, km, rm


def _fd_score_bwd(net, evals, sbar, dx):
  """(adjoint of r3, parameter gradient) for the score's adjoint sbar [B, D]: pass (d, +-) computes
  log_prob = -|x|^2 / 2 + ildj and has the weight +- sbar_d / dx"""
  B = sbar.shape[0]
  r3b, grad = np.zeros_like(sbar), np.zeros(net.n, dtype=net.dt)
  for d, sgn, x, recs in evals:
    w = sgn * sbar[:, d] / dx
    xb, g = _backward(net, recs, -x * w[:, None], w, True, B)
    grad += g
    r3b += xb
  return r3b, grad


def score_ref(cfg, flat, pts, c, dtype=np.float64):
  """cnf_score: (grad_x log_prob [B, D], log_prob [B]) -- the input adjoint of the data -> base pass seeded with (-z, 1)"""
  net = _Net(cfg, flat, dtype)
  pts = np.asarray(pts, dtype=dtype)
  B, D = pts.shape
  z, ld, recs, _, _ = _forward(net, pts, expand_c(c, B, dtype), True)
  xbar, _ = _backward(net, recs, -z, np.ones(B, dtype=dtype), True, B)
  return xbar, -(z * z).sum(1) / 2 - np.asarray(0.5 * D * np.log(2 * np.pi), dtype=dtype) + ld


def logprob_fd_vjp_ref(cfg, flat, pts, c, dx, gbar, dtype=np.float64):
  """cnf_logprob_fd and cnf_logprob_fd_vjp: (score [B, D], pts_bar [B, D], grad)"""
  net = _Net(cfg, flat, dtype)
  pts = np.asarray(pts, dtype=dtype)
  score, evals, _, _ = _fd_score(net, pts, expand_c(c, pts.shape[0], dtype), np.asarray(dx, dtype=dtype))
  pb, grad = _fd_score_bwd(net, evals, np.asarray(gbar, dtype=dtype), np.asarray(dx, dtype=dtype))
  return score, pb, grad


def score_fd_vjp_ref(cfg, flat, r, c, count, dt, dx, coef, drift, a, loss_coef, dtype=np.float64):
  """cnf_score_fd_vjp: (sums [n / count], rbar [3 n, D], grad) for given samples r = [r1 | r2 | r3] -- the gradient
  flows through the 2 D evaluation points of r3 only; drift: a CnfDrift code or -1"""
  net = _Net(cfg, flat, dtype)
  r = np.asarray(r, dtype=dtype)
  n, D = r.shape[0] // 3, r.shape[1]
  f = lambda v: np.asarray(v, dtype=dtype)
  score, evals, _, _ = _fd_score(net, r[2 * n:], expand_c(c, n, dtype), f(dx))
  r64, s64 = r.astype(np.float64), score.astype(np.float64)
  _, rbar, sbar = score_residual_ref(r64, s64, n, count, D, float(dt), float(coef), DRIFT_NAMES[drift], float(a), float(loss_coef))
  u = f(score_residual_u(r64, s64, n, D, float(dt), float(coef), DRIFT_NAMES[drift], float(a)))
  r3b, grad = _fd_score_bwd(net, evals, f(sbar), f(dx))
  rbar = f(rbar)
  rbar[2 * n:] += r3b
  return slice_sums((u * u).sum(1, dtype=dtype).astype(np.float64), count), rbar, grad


def fd_margins(cfg, flat, pts, c, dx):
  """margins of the 2 D evaluation points pts +- dx/2 e_d of every point"""
  net = _Net(cfg, flat, np.float64)
  pts = np.asarray(pts, dtype=np.float64)
  return _fd_score(net, pts, expand_c(c, pts.shape[0]), dx)[2:]


def kinetic_potential_ref(cfg, flat, z, c, S, dt, c_kin, subtype, a, c_pot, dtype=np.float64):
  """cnf_kinetic_potential_vjp: (kin [S], pot [S] or None, grad) for the one draw z pushed to the conditions
  c = [t - dt/2 | t + dt/2 | t] (2 S, or 3 S with subtype >= 0) as given"""
  net = _Net(cfg, flat, dtype)
  f = lambda v: np.asarray(v, dtype=dtype)
  z, c = f(z), f(c).reshape(-1)
  B = z.shape[0]
  kin, pot = np.zeros(S), (np.zeros(S) if subtype >= 0 else None)
  grad = np.zeros(net.n, dtype=dtype)
  push = lambda cv: _forward(net, z, np.full(B, cv, dtype=dtype), False)
  for s in range(S):
    r1, _, rec1, _, _ = push(c[s])
    r2, _, rec2, _, _ = push(c[S + s])
    v = (r2 - r1) / f(dt)
    kin[s] = (v * v).sum(1).sum(dtype=dtype)
    grad += _backward(net, rec1, -2 * f(c_kin) * v / f(dt), None, False, B)[1]
    grad += _backward(net, rec2, 2 * f(c_kin) * v / f(dt), None, False, B)[1]
    if subtype >= 0:
      r3, _, rec3, _, _ = push(c[2 * S + s])
      pot[s] = _potential(subtype, r3, f(a)).sum(dtype=dtype)
      grad += _backward(net, rec3, f(c_pot) * potential_grad(subtype, r3, f(a)), None, False, B)[1]
  return kin, pot, grad


def _term(cfg, flat, spec, pts, t, B, shared, dtype):
  net = _Net(cfg, flat, dtype)
  pts = np.asarray(pts, dtype=dtype)
  t = np.atleast_1d(np.asarray(t, dtype=dtype))
  sums, grad = np.zeros(t.size), np.zeros(net.n, dtype=dtype)
  km, rm = [], []
  for s in range(t.size):
    val, g, a, b = _term_slice(net, spec, pts if shared else pts[s * B:(s + 1) * B], t[s])
    sums[s] = val.sum(dtype=dtype)
    grad += g
    km.append(a); rm.append(b)
  return sums, grad, np.array(km), np.array(rm)


def term_grad(cfg, flat, spec, pts, t, B, shared, dtype=np.float64):
  """(sums [n_slices], grad [n_params]) of one differentiable CnfTermKind as cnf_loss_terms_grad defines it: per-slice
  sums over the slice's samples, and the gradient of the sum over all slices.  spec: anything with the members of
  CnfLossSpec; pts [B, D] (shared) or [n_slices B, D]; t [n_slices]."""
  return _term(cfg, flat, spec, pts, t, B, shared, dtype)[:2]


def term_margins(cfg, flat, spec, pts, t):
  """(knot margin, ReLU margin) [n_slices, n]: per time of t and point of pts, the smallest over the term's passes"""
  _, _, km, rm = _term(cfg, flat, spec, pts, t, pts.shape[0], True, np.float64)
  return km, rm


# ---- inputs -----------------------------------------------------------------------------------------------------------
def select(knot, relu, rows=None, need=None):
  """Fills `need` slots from the drawn points in order, leaving out those too close to a kink: (indices of the points
  taken, share of the points looked at that were left out).  knot, relu: margins [n], or [R, n] with rows [need] saying
  under which row's conditions (a slice's time) each slot is used."""
  ok = (np.atleast_2d(knot) >= KNOT_MARGIN) & (np.atleast_2d(relu) >= RELU_MARGIN)
  rows = np.zeros(need, dtype=int) if rows is None else np.asarray(rows)
  keep, p = [], 0
  while len(keep) < rows.size:
    assert p < ok.shape[1], "not enough points drawn"
    if ok[rows[len(keep)], p]:
      keep.append(p)
    p += 1
  return np.array(keep), 1.0 - len(keep) / p


def random_params(cfg, scale, seed):
  """cnf_ot_amd.Params.random's vector (float32)"""
  return np.random.default_rng(seed).normal(0.0, scale, oracle.param_count(_cfg(cfg))).astype(np.float32)


def draw_points(rng, n, D, spread=1.3, shift=0.0):
  """float32 [n, D]: three quarters N(shift, spread^2), a quarter with at least one coordinate on a linear tail
  (|x| in [10.2, 13.2])"""
  x = rng.normal(shift, spread, (n, D))
  tail = np.arange(n) % 4 == 3
  on = rng.random((n, D)) < 0.5
  on[np.arange(n), rng.integers(0, D, n)] = True
  far = rng.choice([-1.0, 1.0], (n, D)) * (10.2 + 3.0 * rng.random((n, D)))
  return np.where(tail[:, None] & on, far, x).astype(np.float32)


def bound(g32, g64, factor=8.0, knots=None):
  """What a float32 evaluation may differ from the float64 one by on this tensor: `factor` x the float32 run of this
  module against its float64 run (max over the tensor), plus 1e-7 |g|_inf, plus -- knots: `knot_sensitivity` of the
  tensor -- what rounding the knot positions to float32 moves it by."""
  g64 = np.asarray(g64, dtype=np.float64)
  b = factor * np.abs(np.asarray(g32, dtype=np.float64) - g64).max() + 1e-7 * np.abs(g64).max()
  return b if knots is None else b + float(np.max(knots))




# ---- the cases of test_gpu_flow_adjoint.py (test_flow_adjoint_cpu.py asserts the cap on dropped points for each) ------
def spec_of(kind, subtype=0, dt=0.01, dx=0.01, coef=0.5, a=1.0, T=1.0, beta=4.0):
  """the members of CnfLossSpec as the float32 values the kernels receive"""
  f = lambda v: float(np.float32(v))
  return SimpleNamespace(kind=kind, subtype=subtype, dt=f(dt), dx=f(dx), coef=f(coef), a=f(a), T=f(T), beta=f(beta))


def _scale(D):
  return 0.2 if D <= 3 else 0.25 / np.sqrt(D)


def _pool(B):
  return B + max(40, -(-B // 4))


def _pass_cases():
  """(D, L, B, to_base, condition form, seeds, hardware math, max_blocks): every (D, L) in both directions; batch size,
  condition form, seeds and math rotate through them so that each value meets each dimension"""
  out, i = [], 0
  for D in (1, 2, 3, 4, 14):
    for L in (1, 2, 3) + ((4,) if D == 2 else ()):
      for to_base in (False, True):
        B = (1, 63, 65, 257)[(i + i // 4) % 4]
        cform = ("sample", "bcast", "slices")[(i + i // 3) % 3] if B >= 3 else "bcast"
        seeds = ("both", "y", "ld")[(i // 2 + i // 6) % 3]
        out.append((D, L, B, to_base, cform, seeds, i % 3 != 1, 0))
        i += 1
  # five tiles of 256 on an engine whose slabs (max_blocks = 1: four) leave the grid with fewer workgroups than tiles
  out += [(2, 2, 1100, False, "slices", "both", True, 1), (3, 2, 1100, True, "sample", "both", True, 1)]
  return out


PASS_CASES = _pass_cases()


@functools.lru_cache(maxsize=None)
def pass_case(case):
  """the inputs of a pass case (selected points) and its float64 / float32 references"""
  D, L, B, to_base, cform, seeds, fast, _ = case
  cfg = oracle.OracleConfig(D=D, L=L)
  rng = np.random.default_rng(1000 + PASS_CASES.index(case))
  flat = random_params(cfg, _scale(D), 100 + PASS_CASES.index(case))
  n = _pool(B)
  pool = draw_points(rng, n, D)
  if cform == "sample":
    cp = rng.random(n).astype(np.float32)
    knot, relu = margins(cfg, flat, pool, cp, to_base)
  else:
    cs = rng.random(1 if cform == "bcast" else 3).astype(np.float32)
    m = [margins(cfg, flat, pool, cv, to_base) for cv in cs]
    knot, relu = np.array([a for a, _ in m]), np.array([b for _, b in m])
  keep, dropped = select(knot, relu, np.arange(B) // -(-B // knot.shape[0]) if cform == "slices" else None, B)
  pts = pool[keep]
  c = cp[keep] if cform == "sample" else cs
  c_block = 1 if cform == "sample" else (B if cform == "bcast" else -(-B // 3))
  ybar = rng.normal(size=(B, D)).astype(np.float32) if seeds != "ld" else None
  ldbar = rng.normal(size=B).astype(np.float32) if seeds != "y" else None
  ref = lambda dt=np.float64: pass_vjp(cfg, flat, pts, c, ybar, ldbar, to_base, dt)
  r64 = ref()
  return SimpleNamespace(cfg=cfg, flat=flat, pts=pts, c=c, c_block=c_block, ybar=ybar, ldbar=ldbar, dropped=dropped,
                         r64=r64, r32=ref(np.float32), k64=knot_sensitivity(ref, r64))


def _term_cases():
  """(D, L, spec, B, n_slices, shared, hardware math, scale): all six kinds and every potential / drift at its dimension
  on the dim-2 kernel; the generic-dimension kernel at dims 3 and 14; library math at dim 2"""
  K = [spec_of(KINETIC), spec_of(KINETIC_SCORE), spec_of(FLOW_MATCHING, 0), spec_of(FLOW_MATCHING, 1), spec_of(FLOW_MATCHING, 2),
       spec_of(POTENTIAL, 0), spec_of(POTENTIAL, 1, a=1.5), spec_of(POTENTIAL, 2), spec_of(REVERSE_KL), spec_of(NEG_LOGPROB)]
  out = []
  for i, sp in enumerate(K):
    out.append((2, 2, sp, (65, 257)[i % 2], (1, 3)[(i // 2) % 2], i % 3 != 0, True, (1.0, 0.37)[i % 2]))
  out += [(2, 3, spec_of(NEG_LOGPROB), 257, 3, False, True, 0.37), (2, 1, spec_of(KINETIC), 65, 3, True, True, 1.0)]
  for j, sp in enumerate([spec_of(NEG_LOGPROB), spec_of(REVERSE_KL), spec_of(KINETIC), spec_of(FLOW_MATCHING, 3),
                          spec_of(KINETIC_SCORE), spec_of(POTENTIAL, 1)]):
    out.append((3, 2, sp, (257, 65)[j % 2], (3, 1)[j % 2], j % 2 == 0, True, (0.37, 1.0)[j % 2]))
  for j, sp in enumerate([spec_of(NEG_LOGPROB), spec_of(REVERSE_KL), spec_of(KINETIC), spec_of(POTENTIAL, 0)]):
    out.append((14, 2, sp, (65, 257)[j % 2], (3, 1)[j % 2], j % 2 == 1, True, (1.0, 0.37)[j % 2]))
  for j, sp in enumerate([spec_of(NEG_LOGPROB), spec_of(KINETIC), spec_of(FLOW_MATCHING, 0), spec_of(REVERSE_KL)]):
    out.append((2, 2, sp, (257, 65)[j % 2], (1, 3)[j % 2], j % 2 == 0, False, (0.37, 1.0)[j % 2]))
  # (a score term's 2 D + 3 passes at three times would flag too many of a shared draw: those get their own points)
  return [(D, L, sp, B, S, shared and not (S == 3 and sp.kind in (KINETIC_SCORE, FLOW_MATCHING)), fast, sc)
          for D, L, sp, B, S, shared, fast, sc in out]


TERM_CASES = _term_cases()


def term_case_id(case):
  D, L, sp, B, S, shared, fast, scale = case
  return f"D{D}-L{L}-kind{sp.kind}.{sp.subtype}-B{B}-S{S}-{'shared' if shared else 'own'}-{'hw' if fast else 'ocml'}"


def _term_times(S):
  return np.linspace(0.2, 0.8, S).astype(np.float32) if S > 1 else np.array([0.45], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _term_case(index):
  D, L, sp, B, S, shared, fast, scale = TERM_CASES[index]
  cfg = oracle.OracleConfig(D=D, L=L)
  rng = np.random.default_rng(2000 + index)
  flat = random_params(cfg, _scale(D), 200 + index)
  t = _term_times(S)
  n = B if shared else S * B
  pool = draw_points(rng, _pool(n), D, 1.5, 0.3) if sp.kind == NEG_LOGPROB else rng.normal(size=(_pool(n), D)).astype(np.float32)
  knot, relu = term_margins(cfg, flat, sp, pool, t)      # [S, n]: every pass of the term at each time
  if shared:                                             # a shared point is dropped if any of the times flags it
    keep, dropped = select(knot.min(0), relu.min(0), None, n)
  else:
    keep, dropped = select(knot, relu, np.arange(n) // B)
  pts = pool[keep]
  ref = lambda dt=np.float64: term_grad(cfg, flat, sp, pts, t, B, shared, dt)
  r64 = ref()
  return SimpleNamespace(cfg=cfg, flat=flat, pts=pts, t=t, dropped=dropped, r64=r64, r32=ref(np.float32),
                         k64=knot_sensitivity(ref, r64))


def term_case(case):
  return _term_case(TERM_CASES.index(case))


# cnf_score, cnf_logprob_fd_vjp, cnf_score_fd_vjp: (D, L, slices, points per slice -- no multiple of 64, drift, the two
# difference kernels too).  At dim 10 a point's 20 evaluation points pass 20 x 18 conditioners: with two flow layers
# 9 % of a normal draw come within 1e-5 of one of those 11 520 ReLUs, with one layer 4 % -- so the difference kernels
# are held to the reference on one layer there, cnf_score (one pass per point) on both.
SCORE_CASES = [(2, 2, 3, 75, 0, True), (3, 2, 2, 101, -1, True), (10, 1, 2, 45, 0, True), (10, 2, 2, 45, 0, False)]


@functools.lru_cache(maxsize=None)
def score_case(case):
  D, L, S, count, drift, fd = case
  cfg = oracle.OracleConfig(D=D, L=L)
  k = SCORE_CASES.index(case)
  rng = np.random.default_rng(3000 + k)
  flat = random_params(cfg, 0.2 if D == 2 else 0.12, 300 + k)
  t = np.linspace(0.15, 0.85, S).astype(np.float32)
  n, dx, dt = S * count, float(np.float32(0.01)), float(np.float32(0.01))
  pool = (rng.normal(size=(_pool(n), D)) * 1.2).astype(np.float32)
  m = [margins(cfg, flat, pool, cv, True) for cv in t]
  if fd:
    m = [(np.minimum(a, a2), np.minimum(b, b2)) for (a, b), (a2, b2) in zip(m, [fd_margins(cfg, flat, pool, cv, dx) for cv in t])]
  keep, dropped = select(np.array([a for a, _ in m]), np.array([b for _, b in m]), np.arange(n) // count)
  r3 = pool[keep]
  gbar = rng.normal(size=(n, D)).astype(np.float32)
  r12 = (r3[None] + 0.01 * rng.normal(size=(2, n, D))).astype(np.float32)      # stand-ins for the samples at t -+ dt/2
  r = np.concatenate([r12[0], r12[1], r3])
  coef, a, loss_coef = float(np.float32(0.5)), float(np.float32(1.3)), float(np.float32(0.7 / n))
  c = np.repeat(t, count)
  out = SimpleNamespace(cfg=cfg, flat=flat, r3=r3, r=r, t=t, gbar=gbar, dx=dx, dt=dt, coef=coef, a=a, loss_coef=loss_coef,
                        dropped=dropped)
  def ref(dtp=np.float64):
    res = {"score": score_ref(cfg, flat, r3, c, dtp)}
    if fd:
      res["fd"] = logprob_fd_vjp_ref(cfg, flat, r3, c, dx, gbar, dtp)
      res["fused"] = score_fd_vjp_ref(cfg, flat, r, c, count, dt, dx, coef, drift, a, loss_coef, dtp)
    return res

  r64 = ref()
  out.r64, out.r32, out.k64 = SimpleNamespace(**r64), SimpleNamespace(**ref(np.float32)), SimpleNamespace(**knot_sensitivity(ref, r64))
  return out


# the table backward at dim 2: (L, slices, slice length -- just under / just over its tile of 1 024, even)
TABLE_CASES = [(2, 1, 1022), (2, 3, 1026), (3, 3, 1022), (3, 1, 1026)]


@functools.lru_cache(maxsize=None)
def table_case(case):
  L, S, Bs = case
  cfg = oracle.OracleConfig(D=2, L=L)
  k = TABLE_CASES.index(case)
  rng = np.random.default_rng(4000 + k)
  flat = random_params(cfg, 0.2, 400 + k)
  t = np.linspace(0.1, 0.9, S).astype(np.float32) if S > 1 else np.array([0.4], dtype=np.float32)
  B = S * Bs
  dt = float(np.float32(0.01))
  half = np.float32(0.5) * np.float32(0.01)
  c3 = np.concatenate([t - half, t + half, t]).astype(np.float32)
  data = draw_points(rng, _pool(B), 2, 1.3)
  z = rng.normal(size=(_pool(Bs), 2)).astype(np.float32)
  out = SimpleNamespace(cfg=cfg, flat=flat, t=t, c3=c3, dt=dt, coef=float(np.float32(0.013)), c_kin=float(np.float32(0.37 / Bs)),
                        c_pot=float(np.float32(0.11 / Bs)), a=1.5, dropped={})
  sel = {}
  for to_base, pool in ((True, data), (False, data)):
    m = [margins(cfg, flat, pool, cv, to_base) for cv in t]
    sel[to_base], out.dropped[f"pass{int(to_base)}"] = select(np.array([a for a, _ in m]), np.array([b for _, b in m]), np.arange(B) // Bs)
  m = [margins(cfg, flat, z, cv, False) for cv in c3]
  keep, out.dropped["kinpot"] = select(np.min([a for a, _ in m], 0), np.min([b for _, b in m], 0), None, Bs)
  out.z = z[keep]
  out.pts = {tb: data[sel[tb]] for tb in (False, True)}
  out.ybar = rng.normal(size=(B, 2)).astype(np.float32)
  out.ldbar = rng.normal(size=B).astype(np.float32)
  nl = spec_of(NEG_LOGPROB)
  def ref(dtp=np.float64):
    s, g = term_grad(cfg, flat, nl, out.pts[True], t, Bs, False, dtp)
    return {"passes": {tb: pass_vjp(cfg, flat, out.pts[tb], t, out.ybar, out.ldbar, tb, dtp) for tb in (False, True)},
            "neg_logprob": (s, g * np.asarray(out.coef, dtype=dtp)),
            "kinpot": {sub: kinetic_potential_ref(cfg, flat, out.z, c3[:(3 if sub >= 0 else 2) * S], S, dt, out.c_kin, sub,
                                                  out.a, out.c_pot, dtp) for sub in (-1, 1)}}

  r64 = ref()
  out.r64, out.r32, out.k64 = SimpleNamespace(**r64), SimpleNamespace(**ref(np.float32)), SimpleNamespace(**knot_sensitivity(ref, r64))
  return out


@functools.lru_cache(maxsize=None)
def multi_case():
  """cnf_loss_terms_grad_multi: four jobs of different kinds, batch sizes and coefficients on one dim-2 model; the
  reference is the sum of the four terms' gradients.  jobs: [(spec, pts, t, B, shared, scale)]"""
  cfg = oracle.OracleConfig(D=2)
  rng = np.random.default_rng(5000)
  flat = random_params(cfg, 0.2, 500)
  plan = [(spec_of(NEG_LOGPROB), 257, 1, True, 1.0), (spec_of(KINETIC), 65, 3, False, 0.5),
          (spec_of(POTENTIAL, 2), 129, 1, True, 0.25), (spec_of(KINETIC_SCORE), 65, 1, True, 2.0)]
  jobs, dropped = [], []
  for sp, B, S, shared, scale in plan:
    t = _term_times(S)
    n = B if shared else S * B
    pool = draw_points(rng, _pool(n), 2, 1.5, 0.3) if sp.kind == NEG_LOGPROB else rng.normal(size=(_pool(n), 2)).astype(np.float32)
    knot, relu = term_margins(cfg, flat, sp, pool, t)
    keep, d = select(knot.min(0), relu.min(0), None, n) if shared else select(knot, relu, np.arange(n) // B)
    jobs.append((sp, pool[keep], t, B, shared, scale))
    dropped.append(d)
  out = SimpleNamespace(cfg=cfg, flat=flat, jobs=jobs, dropped=max(dropped))
  def ref(dtp=np.float64):
    res = [term_grad(cfg, flat, sp, pts, t, B, shared, dtp) for sp, pts, t, B, shared, _ in jobs]
    return tuple(s for s, _ in res), sum(np.asarray(j[5], dtype=dtp) * g for j, (_, g) in zip(jobs, res))

  out.r64, out.r32 = ref(), ref(np.float32)
  out.k64 = knot_sensitivity(ref, out.r64)
  return out
