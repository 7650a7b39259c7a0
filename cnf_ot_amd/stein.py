"""The kernel Stein discrepancy of a point set against a law known through its score s = grad log p alone -- what
compares an ensemble, or the flow's samples, with a target that has no samples and no normalised density: the particle
references against a closed-form or the flow's exact score, a stationarity residual, a Gibbs law known up to its
constant.  One fused call over all sets (cnf_stein); composed in torch the same pair sum materialises
several N x N matrices and their backward.  Its wild-bootstrap test (cnf_stein_boot) reads the value
as a p-value: the statistic under up to 1 024 Rademacher sign vectors in one pass over the pairs, on the matrix cores.
What surrounds a call is `two_sample`'s.  `utils` re-exports the public names.
"""
import math

import numpy as np
import torch

from . import _capi
from .flows import _OnDevice, _stream_ptr
from .two_sample import (_F32_MIN, _fits, _floats32, _per_64_sets, _ptr, _sets, _stage, _unstack, _workspace,
                         _workspace_bytes, median_bandwidths, pack_labels, permutation_p_value)

STEIN_KINDS = tuple(_capi.STEIN_KINDS)
STEIN_MAX_TERMS, STEIN_MAX_POINTS = _capi.STEIN_MAX_TERMS, 1 << 20
STEIN_BOOT_MIN_VECTORS, STEIN_BOOT_MAX_VECTORS = 32, 1024


def _pow(b, e):
  try:
    return b ** e
  except OverflowError:
    return math.inf


def stein_spec(kind="imq", bandwidths=(1.0,), beta=-0.5, weights=None):
  """The CnfSteinSpec of a base kernel k(x, y) = phi(|x - y|^2) -- ValueError for what cnf_stein refuses in a spec:
    kind="imq":       phi = sum_b weights[b] (bandwidths[b]^2 + r^2)^beta, -1 < beta < 0: the kernel for which the
                      discrepancy controls weak convergence
    kind="gaussian":  phi = sum_b weights[b] exp(-r^2 / (2 bandwidths[b]^2))  (beta is not used)
  1..4 bandwidths, positive and finite as float32; weights positive and finite (None: 1.0 each), one per bandwidth;
  the coefficients of phi''' at a coincident pair (w c^(2 beta - 6); w / (8 h^6)) and c^2, 1 / c^2 in float32's range."""
  if kind not in _capi.STEIN_KINDS:
    raise ValueError(f"ksd: kind is one of {STEIN_KINDS}, not {kind!r}")
  bws = _floats32(bandwidths)
  ws = [1.0] * len(bws) if weights is None else _floats32(weights)
  if not 1 <= len(bws) <= STEIN_MAX_TERMS or len(ws) != len(bws):
    raise ValueError(f"ksd: between 1 and {STEIN_MAX_TERMS} terms, a weight and a bandwidth each, not {len(ws)} weights "
                     f"and {len(bws)} bandwidths")
  be = float(np.float32(beta))
  if kind == "imq" and not -1.0 < be < 0.0:
    raise ValueError(f"ksd: beta must lie in (-1, 0), not {beta}")
  for w, b in zip(ws, bws):
    if not (w > 0.0 and math.isfinite(w)):
      raise ValueError(f"ksd: every weight must be positive and finite (in float32): {ws}")
    if not (b > 0.0 and math.isfinite(b)):
      raise ValueError(f"ksd: every bandwidth must be positive and finite (in float32): {bws}")
    if kind == "imq":
      c2 = b * b
      ok = (_fits(c2) and c2 >= _F32_MIN and _fits(1.0 / c2) and _fits(w * _pow(c2, be))
            and _fits(w * be * (be - 1.0) * (be - 2.0) * _pow(c2, be - 3.0)))
    else:
      ok = b * b > 0.0 and _fits(1.0 / (2.0 * b * b)) and _fits(w * _pow(2.0 * b * b, -3.0))
    if not ok:
      raise ValueError(f"ksd: a coefficient of the kernel's third derivative leaves float32's range: weight {w}, "
                       f"bandwidth {b}")
  spec = _capi.CnfSteinSpec()
  spec.kind, spec.n_terms, spec.beta = _capi.STEIN_KINDS[kind], len(bws), be if kind == "imq" else 0.0
  for i, (w, b) in enumerate(zip(ws, bws)):
    spec.w[i], spec.bw[i] = w, b
  return spec


def stein_phi0(spec):
  """phi(0) of a spec, in float64: the diagonal's and the direction's coefficient"""
  if spec.kind == _capi.STEIN_KINDS["gaussian"]:
    return sum(float(spec.w[b]) for b in range(spec.n_terms))
  return sum(float(spec.w[b]) * (float(spec.bw[b]) ** 2) ** float(spec.beta) for b in range(spec.n_terms))


def stein_check_shapes(x_shape, score_shape=None):
  """ValueError for what cnf_stein refuses: points [S, N, D] with S in 1..64, N in 2..2^20, D in 1..14 and a score of
  another shape."""
  S, N, D = x_shape
  if not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or not 2 <= N <= STEIN_MAX_POINTS:
    raise ValueError(f"ksd: needs 1..{_capi.MMD_MAX_SETS} sets of 2..2^20 points of dimension 1..{_capi.MMD_MAX_DIM}, not "
                     f"{tuple(x_shape)}")
  if score_shape is not None and tuple(score_shape) != tuple(x_shape):
    raise ValueError(f"ksd: the score must have the points' shape {tuple(x_shape)}, not {tuple(score_shape)}")


def _call(spec, x3, s3, want_rows, want_grad):
  """ONE cnf_stein call on staged tensors: (sums [S, 2], rows [S, N] or None, grad_x, grad_s [S, N, D] or None)."""
  S, N, D = x3.shape
  dev = x3.device
  ws = _workspace(dev, _workspace_bytes("cnf_stein_workspace", S, N, D, 1 if want_grad else 0))
  sums = torch.empty(S, 2, dtype=torch.float64, device=dev)
  rows = torch.empty(S, N, dtype=torch.float32, device=dev) if want_rows else None
  gx = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  gs = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_stein(_capi.ctypes.byref(spec), S, x3.data_ptr(), s3.data_ptr(), N, D, sums.data_ptr(),
                                      _ptr(rows), _ptr(gx), _ptr(gs), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                "cnf_stein")
  return sums, rows, gx, gs


def ksd_of_sets(spec, x3, s3, want_grad):
  """(KSD^2_U [S] float64, grad_x, grad_s [S, N, D] or None) of staged sets with any S: ONE cnf_stein call per 64 sets."""
  N = x3.shape[1]
  sums, _, gx, gs = _per_64_sets(lambda x, s: _call(spec, x, s, False, want_grad), x3, s3)
  return sums[:, 0] / (N * (N - 1.0)), gx, gs


def ksd(x, score, kind="imq", bandwidths=None, beta=-0.5, weights=None, want_grad=False, want_rows=False) -> dict:
  """The kernel Stein discrepancy of the point sets x [N, D] or [S, N, D] against the law whose score grad log p at those
  points is `score` (x's shape), for the base kernel of `stein_spec` (bandwidths=None: median_bandwidths(x), first 4),
  ONE fused cnf_stein call over all sets (the pair i == j is skipped by index; duplicated points at other indices do
  interact).  float32 on the device (float64 inputs are rounded; host inputs are uploaded).  Returns a dict:
    ksd2 [S]     the U-statistic sum_{i != j} k_p / (N (N - 1)) (float64): unbiased, 0 in the mean iff x ~ p
    ksd2_v [S]   the V-statistic sum_{i, j} k_p / N^2 >= 0
    sums [S, 2]  the raw sum_{i != j} k_p and sum_i k_p(x_i, x_i)
    rows         want_rows: [S, N] float32 ([N] for 2-D x), sum_{j != i} k_p / (N - 1): each point's share; else None
    grad_x, grad_score   want_grad: [S, N, D] float32 ([N, D] for 2-D x), the gradients of ksd2 in x and in the score,
                 the score held an independent input; else None
    direction    want_grad: the Stein variational direction mean_j (k(x_j, x_i) score_j + grad_{x_j} k(x_j, x_i)) =
                 ((N - 1) / 2) grad_score + phi(0) score / N, shaped like grad_x; else None
    bandwidths   the list used
  Two calls give the same bits, and sums do not depend on the want_ flags.  ValueError before any device work for what
  the C ABI refuses."""
  x3, s3 = _sets("ksd", x, "x"), _sets("ksd", score, "score")
  stein_check_shapes(x3.shape, s3.shape)
  if bandwidths is None:
    bandwidths = median_bandwidths(x3)[:STEIN_MAX_TERMS]
  spec = stein_spec(kind, bandwidths, beta, weights)
  N = x3.shape[1]
  dev, one, (x3, s3) = _stage(x, x3, s3)
  sums, rows, gx, gs = _call(spec, x3, s3, want_rows, want_grad)
  direction = None if gs is None else gs * (0.5 * (N - 1.0)) + s3 * (stein_phi0(spec) / N)
  return {"ksd2": sums[:, 0] / (N * (N - 1.0)), "ksd2_v": (sums[:, 0] + sums[:, 1]) / (float(N) * N), "sums": sums,
          "rows": _unstack(rows, one), "grad_x": _unstack(gx, one), "grad_score": _unstack(gs, one),
          "direction": _unstack(direction, one), "bandwidths": [float(spec.bw[i]) for i in range(spec.n_terms)]}


# ---- the wild-bootstrap test of the Stein discrepancy ------------------------------------------------------------------
# With H the zero-diagonal Stein kernel matrix and e a vector of fair signs, e' H e / (N (N - 1)) has, under x ~ p, the
# law of KSD^2_U itself (the U-statistic is degenerate there): its quantiles are the test's.  One fused pass forms every
# pair value once for all sign vectors (cnf_stein_boot).

def rademacher_signs(N, n_boot, seed=0):
  """The sign words of a wild-bootstrap test of N points, an int32 CPU tensor [N, (n_boot + 1) / 32]: bit b of word w of
  point j is set where e_j = +1 under sign vector 32 w + b.  Vector 0 is all +1 (the observed statistic); vectors
  1..n_boot are fair bits drawn by numpy's default_rng(seed) -- a fixed function of (N, n_boot, seed).  ValueError unless
  n_boot + 1 is a multiple of 32 within 32..1024 and N >= 1."""
  N, P = int(N), int(n_boot) + 1
  if P % 32 or not STEIN_BOOT_MIN_VECTORS <= P <= STEIN_BOOT_MAX_VECTORS:
    raise ValueError(f"rademacher_signs: n_boot + 1 must be a multiple of 32 within {STEIN_BOOT_MIN_VECTORS}.."
                     f"{STEIN_BOOT_MAX_VECTORS}, not {P}")
  if N < 1:
    raise ValueError(f"rademacher_signs: needs N >= 1, not {N}")
  plus = np.random.default_rng(int(seed)).integers(0, 2, size=(N, P), dtype=np.uint8).astype(bool)
  plus[:, 0] = True
  return pack_labels(plus)


def stein_boot_check_shapes(x_shape, score_shape=None, signs_shape=None):
  """ValueError for what cnf_stein_boot refuses: ([S, N, D], [S, N, D], [N, W]) with S in 1..64, N in 2..2^20, D in 1..14,
  a score of the points' shape and W = P / 32 words in 1..32."""
  stein_check_shapes(x_shape, score_shape)
  N = x_shape[1]
  if signs_shape is not None and (len(signs_shape) != 2 or signs_shape[0] != N
                                  or not 1 <= signs_shape[1] <= STEIN_BOOT_MAX_VECTORS // 32):
    raise ValueError(f"ksd_bootstrap: signs must be [{N}, P / 32] words with P in {STEIN_BOOT_MIN_VECTORS}.."
                     f"{STEIN_BOOT_MAX_VECTORS}, not {tuple(signs_shape)}")


def ksd_bootstrap_test(x, score, kind="imq", bandwidths=None, beta=-0.5, weights=None, n_boot=255, seed=0,
                       signs=None) -> dict:
  """The wild-bootstrap goodness-of-fit test of the point sets x [N, D] or [S, N, D] against the law whose score at those
  points is `score` (x's shape; kernel as `ksd`, bandwidths=None: median_bandwidths(x), first 4): KSD^2_U under n_boot
  vectors of fair signs, ONE cnf_stein_boot call per 64 sets.  signs: the sign words [N, P / 32] (None:
  rademacher_signs(N, n_boot, seed)); with signs given, n_boot = P - 1 and vector 0 is taken as the observed statistic
  (all +1).  The same sign vectors serve all sets.  The points are taken as independent draws: for exchangeable or
  correlated points (interacting particles, a chain) this bootstrap does not apply.  float32 on the device.  Returns a
  dict:
    ksd2 [S]           sign vector 0's statistic e' H e / (N (N - 1)) (float64): KSD^2_U
    null [S, n_boot]   the statistic under vectors 1..n_boot
    p_value [S]        (1 + #{null >= ksd2}) / (1 + n_boot)
    ksd2_v, null_v, p_value_v   the same for the V-statistic (e' H e + sum_i k_p(x_i, x_i)) / N^2
    raw                {"q": [S, P], "t": [S], "diag": [S]}: e' H e, 1' H 1 and the diagonal sum, from which every value
                       can be audited
    bandwidths         the list used
  Evaluation only: no gradient.  Two calls give the same bits.  ValueError before any device work for what the C ABI
  refuses and for x, score and signs that do not fit together."""
  x3, s3 = _sets("ksd_bootstrap", x, "x"), _sets("ksd_bootstrap", score, "score")
  S, N, D = x3.shape
  one_call = (min(S, _capi.MMD_MAX_SETS), N, D)    # (any S: 64 sets per call)
  stein_boot_check_shapes(one_call, (min(s3.shape[0], _capi.MMD_MAX_SETS),) + tuple(s3.shape[1:]))
  if s3.shape[0] != S:
    raise ValueError(f"ksd_bootstrap: the score must have the points' shape {tuple(x3.shape)}, not {tuple(s3.shape)}")
  if signs is None:
    signs = rademacher_signs(N, n_boot, seed)
  signs = signs if torch.is_tensor(signs) else torch.as_tensor(np.asarray(signs))
  stein_boot_check_shapes(one_call, None, tuple(signs.shape))
  if signs.dtype != torch.int32:
    raise ValueError(f"ksd_bootstrap: signs are int32 words, not {signs.dtype}")
  P = 32 * signs.shape[1]
  if bandwidths is None:
    bandwidths = median_bandwidths(x3)[:STEIN_MAX_TERMS]
  spec = stein_spec(kind, bandwidths, beta, weights)
  dev, _, (x3, s3) = _stage(x, x3, s3)
  words = signs.detach().to(device=dev).contiguous()

  def call(xc, sc):
    Sc = xc.shape[0]
    ws = _workspace(dev, _workspace_bytes("cnf_stein_boot_workspace", Sc, N, D, P))
    stats = torch.empty(Sc, P, dtype=torch.float64, device=dev)
    raw = torch.empty(Sc * (P + 2), dtype=torch.float64, device=dev)
    with _OnDevice(dev):
      _capi.check(_capi.lib().cnf_stein_boot(_capi.ctypes.byref(spec), Sc, xc.data_ptr(), sc.data_ptr(), N, D,
                                             words.data_ptr(), P, stats.data_ptr(), raw.data_ptr(), ws.data_ptr(),
                                             ws.numel() * 8, _stream_ptr(dev)), "cnf_stein_boot")
    return stats, raw[:Sc * P].view(Sc, P), raw[Sc * P:Sc * (P + 1)], raw[Sc * (P + 1):]

  stats, q, t, diag = _per_64_sets(call, x3, s3)
  stats_v = (q + diag[:, None]) / (float(N) * N)
  return {"ksd2": stats[:, 0], "null": stats[:, 1:], "p_value": permutation_p_value(stats[:, 0], stats[:, 1:]),
          "ksd2_v": stats_v[:, 0], "null_v": stats_v[:, 1:], "p_value_v": permutation_p_value(stats_v[:, 0], stats_v[:, 1:]),
          "raw": {"q": q, "t": t, "diag": diag}, "bandwidths": [float(spec.bw[i]) for i in range(spec.n_terms)]}
