"""The mean-field interaction energy of a point cloud -- the one cost of a mean-field control problem that is not
local in the density: F[rho] = 1/2 int int W(x - y) rho(x) rho(y) dx dy on samples, its first variation W * rho (a
field) and its Wasserstein gradient grad (W * rho) (a force), for a signed Gaussian, exponential (Morse), quadratic or
softened power-law / log pair kernel W(|x - y|).  One fused call over all sets (cnf_interaction);
composed in torch the same double sum materialises an N x N matrix per set and its backward.  `interaction_force_vjp`
is the backward of the force itself (cnf_interaction_vjp): what a loss needs that has the force inside
a square, as the interacting Fokker-Planck residual does.  What surrounds a call is `two_sample`'s.  `utils` re-exports
the public names.
"""
import math

import numpy as np
import torch

from . import _capi
from .flows import _OnDevice, _stream_ptr
from .two_sample import _fits, _per_64_sets, _ptr, _sets, _stage, _unstack, _workspace, _workspace_bytes

INTERACTION_KINDS = tuple(_capi.INTERACTION_KINDS)
INTERACTION_MAX_TERMS, INTERACTION_MAX_POINTS = _capi.INTERACTION_MAX_TERMS, _capi.INTERACTION_MAX_POINTS


def _floats(v):
  return [float(b) for b in np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)]


def _pow(eps, e):
  """eps^e as the C ABI's check forms it (std::pow): eps^0 = 1 also at eps = 0, inf where eps = 0 meets e < 0, and inf
  where the power leaves float64"""
  if e == 0.0:
    return 1.0
  if eps == 0.0:
    return math.inf if e < 0.0 else 0.0
  try:
    return eps ** e
  except OverflowError:
    return math.inf


def _power_spec(spec, amplitudes, bandwidths, exponents):
  """interaction_spec for kind="power": the checks of ia_coef_power (csrc/cnf_interaction_pairs.h), on the float32
  values the kernel sees"""
  if exponents is None:
    raise ValueError("interaction: the power kind needs its exponents")
  pws = [float(np.float32(p)) for p in _floats(exponents)]
  amps = [1.0] * len(pws) if amplitudes is None else [float(np.float32(a)) for a in _floats(amplitudes)]
  if not 1 <= len(pws) <= INTERACTION_MAX_TERMS or len(amps) != len(pws):
    raise ValueError(f"interaction: between 1 and {INTERACTION_MAX_TERMS} terms, an amplitude and an exponent each, not "
                     f"{len(amps)} amplitudes and {len(pws)} exponents")
  eps = [0.0] if bandwidths is None else _floats(bandwidths)
  if len(eps) != 1:
    raise ValueError(f"interaction: the power kind has ONE softening length (bandwidths), not {len(eps)}")
  eps = float(np.float32(eps[0]))
  if not (math.isfinite(eps) and eps >= 0.0 and _fits(eps * eps)):
    raise ValueError(f"interaction: the softening length must be finite and >= 0 (in float32, with its square): {eps}")
  for a, p in zip(amps, pws):
    if not (math.isfinite(a) and a != 0.0):
      raise ValueError(f"interaction: every amplitude must be non-zero and finite (in float32): {amps}")
    if not (math.isfinite(p) and abs(p) <= _capi.INTERACTION_MAX_EXPONENT):
      raise ValueError(f"interaction: every exponent must be finite with |p| <= {_capi.INTERACTION_MAX_EXPONENT:g}: "
                       f"{pws}")
    if eps == 0.0 and not p >= 2.0:
      raise ValueError(f"interaction: a softening length of 0 needs every exponent >= 2 (a singular kernel otherwise): "
                       f"{pws}")
    value = a * math.log(eps) if p == 0.0 else (a / p) * _pow(eps, p)
    partial = 0.0 if p == 0.0 else (a / p) * _pow(eps, p - 2.0)      # (the value's sum before its factor u)
    if not (_fits(a * _pow(eps, p - 2.0)) and _fits(value) and (p == 0.0 or _fits(a / p)) and _fits(partial)):
      raise ValueError(f"interaction: amp eps^(p - 2) (the force) or amp eps^p / p (the value) leaves float32's range: "
                       f"{a}, {p}, eps {eps}")
  spec.n_terms = len(pws)
  for i, (a, p) in enumerate(zip(amps, pws)):
    spec.amp[i], spec.pw[i] = a, p
  spec.bw[0] = eps
  return spec


def interaction_spec(kind, amplitudes=None, bandwidths=None, exponents=None):
  """The CnfInteractionSpec of a pair kernel -- ValueError for what cnf_interaction refuses in a spec:
    kind="gaussian":     W(r) = sum_b amplitudes[b] exp(-r^2 / (2 bandwidths[b]^2))
    kind="exponential":  W(r) = sum_b amplitudes[b] exp(-r / bandwidths[b])  (Morse: amplitudes (C_r, -C_a))
    kind="quadratic":    W(r) = amplitudes[0] r^2 / 2  (bandwidths are not used)
    kind="power":        W(r) = sum_b amplitudes[b] u^(exponents[b] / 2) / exponents[b], u = r^2 + eps^2, a term with
                         exponent 0 being amplitudes[b] ln(u) / 2 (the log kernel): grad W = (x - y) sum_b amplitudes[b]
                         u^(exponents[b] / 2 - 1).  eps = bandwidths, ONE softening length (None: 0, allowed only with
                         every exponent >= 2).  Coulomb / Newton in dimension D: exponents=[2 - D] (D = 2: [0]),
                         amplitude < 0 for repulsion (W = amp u^(p / 2) / p, p < 0); attraction-repulsion r^a / a -
                         r^b / b: exponents=[a, b], amplitudes=[1, -1]
  Amplitudes are signed, non-zero and finite (None: 1.0 each); 1..4 bandwidths (None: 1.0), positive and finite as
  float32 with 1 / bw^2, and amp / bw^2 (Gaussian) or amp / bw (exponential), in float32's range.  Power: 1..4 exponents,
  finite with |p| <= 16, one amplitude each; eps finite and >= 0; amp eps^(p - 2) and amp eps^p / p in float32's range.
  `exponents` belong to the power kind alone."""
  if kind not in _capi.INTERACTION_KINDS:
    raise ValueError(f"interaction: kind is one of {INTERACTION_KINDS}, not {kind!r}")
  spec = _capi.CnfInteractionSpec()
  spec.kind = _capi.INTERACTION_KINDS[kind]
  if kind == "power":
    return _power_spec(spec, amplitudes, bandwidths, exponents)
  if exponents is not None:
    raise ValueError(f"interaction: exponents belong to the power kind, not to {kind!r}")
  if kind == "quadratic":
    amps = [1.0] if amplitudes is None else _floats(amplitudes)
    if len(amps) != 1:
      raise ValueError(f"interaction: the quadratic kind has one amplitude, not {len(amps)}")
    bws = []
  else:
    bws = [1.0] * (1 if amplitudes is None else len(_floats(amplitudes))) if bandwidths is None else _floats(bandwidths)
    amps = [1.0] * len(bws) if amplitudes is None else _floats(amplitudes)
    if not 1 <= len(bws) <= INTERACTION_MAX_TERMS or len(amps) != len(bws):
      raise ValueError(f"interaction: between 1 and {INTERACTION_MAX_TERMS} terms, an amplitude and a bandwidth each, not "
                       f"{len(amps)} amplitudes and {len(bws)} bandwidths")
  for a in amps:
    a32 = float(np.float32(a))
    if not (np.isfinite(a32) and a32 != 0.0):
      raise ValueError(f"interaction: every amplitude must be non-zero and finite (in float32): {amps}")
  for a, b in zip(amps, bws):
    a32, b32 = float(np.float32(a)), float(np.float32(b))      # (as the kernel sees them)
    if not (b32 > 0.0 and np.isfinite(b32) and 1.0 / (b32 * b32) <= 3.0e38):
      raise ValueError(f"interaction: every bandwidth must be positive and finite (in float32, with 1 / bw^2): {bws}")
    ib = 1.0 / (b32 * b32) if kind == "gaussian" else 1.0 / b32
    if not abs(a32 * ib) <= 3.4028234663852886e38:
      raise ValueError(f"interaction: amplitude / bandwidth{'^2' if kind == 'gaussian' else ''} leaves float32's range: "
                       f"{a}, {b}")
  spec.n_terms = max(1, len(bws))
  for i, a in enumerate(amps):
    spec.amp[i] = a
  for i, b in enumerate(bws):
    spec.bw[i] = b
  return spec


def interaction_check_shapes(x_shape, q_shape=None):
  """ValueError for what cnf_interaction refuses: sources [S, N, D] with S in 1..64, N in 2..2^20, D in 1..14 and, in
  query mode, points [S, Q, D] with Q in 1..2^20."""
  S, N, D = x_shape
  if not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or not 2 <= N <= INTERACTION_MAX_POINTS:
    raise ValueError(f"interaction: needs 1..{_capi.MMD_MAX_SETS} sets of 2..2^20 points of dimension "
                     f"1..{_capi.MMD_MAX_DIM}, not {tuple(x_shape)}")
  if q_shape is not None:
    if len(q_shape) != 3 or q_shape[0] != S or q_shape[2] != D or not 1 <= q_shape[1] <= INTERACTION_MAX_POINTS:
      raise ValueError(f"interaction: the query points must be [{S}, Q, {D}] with Q in 1..2^20, not {tuple(q_shape)}")


def _call(spec, x3, q3, want_pot, want_force):
  """ONE cnf_interaction call on staged tensors: (sums [S], pot [S, rows] or None, force [S, rows, D] or None)."""
  S, N, D = x3.shape
  Q = 0 if q3 is None else q3.shape[1]
  rows, dev = Q or N, x3.device
  ws = _workspace(dev, _workspace_bytes("cnf_interaction_workspace", S, N, Q, D, 1 if want_force else 0))
  sums = torch.empty(S, dtype=torch.float64, device=dev)
  pot = torch.empty(S, rows, dtype=torch.float32, device=dev) if want_pot else None
  force = torch.empty(S, rows, D, dtype=torch.float32, device=dev) if want_force else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_interaction(_capi.ctypes.byref(spec), S, x3.data_ptr(), N, _ptr(q3), Q, D, sums.data_ptr(),
                                            _ptr(pot), _ptr(force), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                "cnf_interaction")
  return sums, pot, force


def energy_of_sets(spec, x3, want_grad):
  """(F [S] float64, dF / dx [S, N, D] or None) of staged sets x3 [S, N, D] with any S: ONE cnf_interaction call per 64
  sets."""
  N = x3.shape[1]
  sums, _, force = _per_64_sets(lambda x: _call(spec, x, None, False, want_grad), x3)
  return sums / (2.0 * N * (N - 1.0)), None if force is None else force * (1.0 / N)


def interaction_energy(x, kind, amplitudes=None, bandwidths=None, want_grad=False, want_field=False,
                       exponents=None) -> dict:
  """The interaction energy F = sum_{i != j} W(x_i - x_j) / (2 N (N - 1)) of the point sets x [N, D] or [S, N, D] for the
  pair kernel of `interaction_spec`, ONE fused cnf_interaction call over all sets (self mode: the pair i == j is
  skipped by index; duplicated points at other indices do interact).  float32 on the device (float64 inputs are
  rounded; host inputs are uploaded).  Returns a dict: energy [S] (float64), sums [S] (the raw double sum) and, with
  want_field, potential [S, N] (float32; [N] for 2-D x) = (W * rho)(x_i) over the other N - 1 points, with want_grad,
  grad [S, N, D] ([N, D] for 2-D x) = dF / dx = the force grad (W * rho)(x_i) / N.  Two calls give the same bits, and
  the energy does not depend on the want_ flags.  ValueError before any device work for what the C ABI refuses."""
  x3 = _sets("interaction", x, "x")
  interaction_check_shapes(x3.shape)
  spec = interaction_spec(kind, amplitudes, bandwidths, exponents)
  N = x3.shape[1]
  dev, one, (x3, _) = _stage(x, x3, x3[:, :0])
  sums, pot, force = _call(spec, x3, None, want_field, want_grad)
  out = {"energy": sums / (2.0 * N * (N - 1.0)), "sums": sums}
  if want_field:
    out["potential"] = _unstack(pot, one)
  if want_grad:
    out["grad"] = _unstack(force * (1.0 / N), one)
  return out


def interaction_field(points, sources, kind, amplitudes=None, bandwidths=None, want_force=True, exponents=None) -> dict:
  """The field of the sources [N, D] or [S, N, D] at the points [Q, D] or [S, Q, D] (set s against set s), ONE fused
  cnf_interaction call in query mode (nothing is skipped): potential [S, Q] (float32; [Q] for 2-D points) =
  (W * rho)(q_i) = mean_j W(q_i - x_j), with want_force force [S, Q, D] = grad (W * rho)(q_i) -- what a particle method
  with this interaction would call per step -- and sums [S] (float64) = sum_i sum_j W.  ValueError before any device
  work for what the C ABI refuses and for points and sources that differ in S or D."""
  q3, x3 = _sets("interaction", points, "points"), _sets("interaction", sources, "sources")
  interaction_check_shapes(x3.shape, tuple(q3.shape))
  spec = interaction_spec(kind, amplitudes, bandwidths, exponents)
  dev, one, (q3, x3) = _stage(points, q3, x3)
  sums, pot, force = _call(spec, x3, q3, True, want_force)
  out = {"potential": _unstack(pot, one), "sums": sums}
  if want_force:
    out["force"] = _unstack(force, one)
  return out


# ---- the force's vector-Jacobian product: what a loss with the force inside a square differentiates through ----------

def interaction_vjp_check_spec(spec):
  """ValueError for what cnf_interaction_vjp refuses in a spec that `interaction_spec` accepted: a pair-Hessian
  coefficient amp / bw^4 (Gaussian), amp / bw^2 (exponential) or amp (p - 2) eps^(p - 4) (power; none for p = 2) outside
  float32's range."""
  if spec.kind == _capi.INTERACTION_KINDS["quadratic"]:
    return spec
  if spec.kind == _capi.INTERACTION_KINDS["power"]:
    eps = float(spec.bw[0])
    for b in range(spec.n_terms):
      a, p = float(spec.amp[b]), float(spec.pw[b])
      if p != 2.0 and not (_fits(a * (p - 2.0) * _pow(eps, p - 4.0)) and _fits(a * (p - 2.0))):
        raise ValueError(f"interaction: amp (p - 2) eps^(p - 4) (the pair Hessian's coefficient) leaves float32's range: "
                         f"{a}, {p}, eps {eps}")
    return spec
  power = 4 if spec.kind == _capi.INTERACTION_KINDS["gaussian"] else 2
  for b in range(spec.n_terms):
    if not abs(float(spec.amp[b]) / float(spec.bw[b]) ** power) <= 3.4028234663852886e38:
      raise ValueError(f"interaction: amplitude / bandwidth^{power} (the pair Hessian's coefficient) leaves float32's "
                       f"range: {float(spec.amp[b])}, {float(spec.bw[b])}")
  return spec


def _vjp_call(spec, x3, g3):
  """ONE cnf_interaction_vjp call on staged tensors: xbar [S, N, D]."""
  S, N, D = x3.shape
  dev = x3.device
  ws = _workspace(dev, _workspace_bytes("cnf_interaction_vjp_workspace", S, N, D))
  xbar = torch.empty(S, N, D, dtype=torch.float32, device=dev)
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_interaction_vjp(_capi.ctypes.byref(spec), S, x3.data_ptr(), g3.data_ptr(), N, D,
                                                xbar.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                "cnf_interaction_vjp")
  return xbar


def force_of_sets(spec, x3):
  """The self-mode force [S, N, D] of staged sets x3 with any S: ONE cnf_interaction call per 64 sets."""
  return _per_64_sets(lambda x: _call(spec, x, None, False, True)[2], x3)


def force_vjp_of_sets(spec, x3, g3):
  """xbar [S, N, D] of staged sets x3 and force adjoints g3 with any S: ONE cnf_interaction_vjp call per 64 sets."""
  return _per_64_sets(lambda x, g: _vjp_call(spec, x, g), x3, g3)


def interaction_force_vjp(x, g, kind, amplitudes=None, bandwidths=None, exponents=None):
  """The vector-Jacobian product of the self-mode force f_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j) of the point
  sets x [N, D] or [S, N, D] (what utils.interaction_energy's grad is, times N) with the adjoint g of the same shape:
    xbar_k = (1 / (N - 1)) sum_{j != k} H(x_k - x_j) (g_k - g_j),   H the pair Hessian of W,
  float32 [S, N, D] ([N, D] for 2-D x), ONE fused cnf_interaction_vjp call per 64 sets; composed in
  torch it is a double backward through an N x N x D pair tensor per set.  It is the exact gradient of sum_i g_i . f_i
  as the kernel computes f: for the exponential kind a coincident pair contributes nothing, and in dimension 1 the
  result does not contain the delta term of the kink of W at 0.  Two calls give the same bits.  ValueError before any
  device work for what the C ABI refuses."""
  x3, g3 = _sets("interaction", x, "x"), _sets("interaction", g, "g")
  interaction_check_shapes((min(x3.shape[0], _capi.MMD_MAX_SETS),) + tuple(x3.shape[1:]))
  if tuple(g3.shape) != tuple(x3.shape):
    raise ValueError(f"interaction: the force's adjoint must have the points' shape {tuple(x3.shape)}, not {tuple(g3.shape)}")
  spec = interaction_vjp_check_spec(interaction_spec(kind, amplitudes, bandwidths, exponents))
  dev, one, (x3, g3) = _stage(x, x3, g3)
  return _unstack(force_vjp_of_sets(spec, x3, g3), one)
