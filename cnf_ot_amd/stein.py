"""The kernel Stein discrepancy of a point set against a law known through its score s = grad log p alone -- what
compares an ensemble, or the flow's samples, with a target that has no samples and no normalised density: the particle
references against a closed-form or the flow's exact score, a stationarity residual, a Gibbs law known up to its
constant.  One fused call over all sets (cnf_stein); composed in torch the same pair sum materialises
several N x N matrices and their backward.  What surrounds a call is `two_sample`'s.  `utils` re-exports the public
names.
"""
import math

import numpy as np
import torch

from . import _capi
from .flows import _OnDevice, _stream_ptr
from .two_sample import (_F32_MIN, _fits, _floats32, _per_64_sets, _ptr, _sets, _stage, _unstack, _workspace,
                         _workspace_bytes, median_bandwidths)

STEIN_KINDS = tuple(_capi.STEIN_KINDS)
STEIN_MAX_TERMS, STEIN_MAX_POINTS = _capi.STEIN_MAX_TERMS, 1 << 20


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
