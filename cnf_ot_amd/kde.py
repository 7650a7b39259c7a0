"""A Gaussian kernel density estimate of a point set in the log domain, with its score -- what turns an ensemble into
FIELDS at given points in the full dimension: log rho and grad log rho of a particle reference, the leave-one-out
likelihood of a bandwidth.  One fused call over all sets and bandwidths (cnf_kde); composed in torch
the same estimate materialises a Q x N matrix per bandwidth.  What surrounds a call is `two_sample`'s.  `utils`
re-exports the public names.
"""
import math

import torch

from . import _capi
from .flows import _OnDevice, _stream_ptr
from .two_sample import _F32_MAX, _F32_MIN, _floats32, _ptr, _sets, _stage, _unstack, _workspace, _workspace_bytes

KDE_MAX_BW, KDE_MAX_POINTS, KDE_BANDWIDTH_ROWS = _capi.KDE_MAX_BW, 1 << 20, 4096

def kde_spec(bandwidths, loo=False):
  """The CnfKdeSpec of 1..4 bandwidths -- ValueError for what cnf_kde refuses in a spec: a bandwidth that is not positive
  and finite as float32, or whose 1 / (2 h^2) is not a normal float32."""
  bws = _floats32(bandwidths)
  if not 1 <= len(bws) <= KDE_MAX_BW:
    raise ValueError(f"kde: between 1 and {KDE_MAX_BW} bandwidths, not {len(bws)}")
  for b in bws:
    if not (b > 0.0 and math.isfinite(b)):
      raise ValueError(f"kde: every bandwidth must be positive and finite (in float32): {bws}")
    if not (b * b > 0.0 and _F32_MIN <= 1.0 / (2.0 * b * b) <= _F32_MAX):
      raise ValueError(f"kde: 1 / (2 h^2) leaves float32's range for the bandwidth {b}")
  spec = _capi.CnfKdeSpec()
  spec.n_bw, spec.loo = len(bws), 1 if loo else 0
  for i, b in enumerate(bws):
    spec.bw[i] = b
  return spec


def kde_check_shapes(x_shape, q_shape=None, loo=False):
  """ValueError for what cnf_kde refuses: sources [S, N, D] with S in 1..64, N in 1..2^20 (2.. with loo), D in 1..14;
  queries [S, Q, D] with Q in 1..2^20 and the sources' S and D; loo with queries of their own."""
  S, N, D = x_shape
  if not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or not (2 if loo else 1) <= N <= KDE_MAX_POINTS:
    raise ValueError(f"kde: needs 1..{_capi.MMD_MAX_SETS} sets of {2 if loo else 1}..2^20 sources of dimension "
                     f"1..{_capi.MMD_MAX_DIM}, not {tuple(x_shape)}")
  if q_shape is None:
    return
  if loo:
    raise ValueError("kde: leave-one-out is self mode's: it takes no points of their own")
  Sq, Q, Dq = q_shape
  if Sq != S or Dq != D or not 1 <= Q <= KDE_MAX_POINTS:
    raise ValueError(f"kde: the points must be [{S}, 1..2^20, {D}] for sources {tuple(x_shape)}, not {tuple(q_shape)}")


def kde_bandwidths(x, rule="silverman", factors=(1.0,)):
  """The normal-reference bandwidths factor * sd * (4 / ((D + 2) N))^(1 / (D + 4)) of the sources x [N, D] or [S, N, D]
  (all sets pooled: a call has one list of bandwidths), a list of len(factors) floats.  sd is the root of the mean
  per-coordinate variance over at most 4 096 rows per set, in torch (float64); N is a set's full count."""
  if rule != "silverman":
    raise ValueError(f"kde_bandwidths: rule is 'silverman', not {rule!r}")
  x = torch.as_tensor(x)
  if x.dim() == 2:
    x = x[None]
  if x.dim() != 3 or x.shape[1] < 2:
    raise ValueError(f"kde_bandwidths: expected [N >= 2, D] or [S, N, D] points, got {tuple(x.shape)}")
  N, D = x.shape[1], x.shape[2]
  sd = math.sqrt(float(x[:, :KDE_BANDWIDTH_ROWS].double().var(dim=1, unbiased=True).mean()))
  if not (sd > 0.0 and math.isfinite(sd)):
    raise ValueError(f"kde_bandwidths: the sources' standard deviation is {sd}")
  return [float(f) * sd * (4.0 / ((D + 2.0) * N)) ** (1.0 / (D + 4.0)) for f in factors]


def _call(spec, x3, q3, want_score):
  """ONE cnf_kde call on staged tensors (q3 None: self mode): (log_rho [S, B, Q], score [S, B, Q, D] or None, sums [S, B])."""
  S, N, D = x3.shape
  Q, B = N if q3 is None else q3.shape[1], spec.n_bw
  dev = x3.device
  ws = _workspace(dev, _workspace_bytes("cnf_kde_workspace", S, N, Q, D, B, 1 if want_score else 0))
  log_rho = torch.empty(S, B, Q, dtype=torch.float32, device=dev)
  score = torch.empty(S, B, Q, D, dtype=torch.float32, device=dev) if want_score else None
  sums = torch.empty(S, B, dtype=torch.float64, device=dev)
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_kde(_capi.ctypes.byref(spec), S, x3.data_ptr(), N, _ptr(q3), Q, D, log_rho.data_ptr(),
                                    _ptr(score), sums.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                "cnf_kde")
  return log_rho, score, sums


def kde(points, sources=None, bandwidths=None, want_score=True, loo=None) -> dict:
  """The Gaussian kernel density estimate of the source sets at `points` ([Q, D] or [S, Q, D]), in the log domain, ONE
  fused cnf_kde call over all sets and bandwidths.  sources=None is self mode: the points are the sources, and loo
  (default True there) leaves the pair j == i out by index, n_eff = N - 1.  With sources ([N, D] or [S, N, D]) loo must
  be falsy.  bandwidths=None: kde_bandwidths(sources).  float32 on the device (float64 inputs are rounded; host inputs
  are uploaded).  Returns a dict:
    log_density [S, B, Q]        float32 ([B, Q] for 2-D points); -inf where no source is within float32's reach
    score [S, B, Q, D]           want_score: float32, grad log of the estimate at the points (0 there); else None
    mean_log_density [S, B]      float64, sum_i log_density / Q: with loo the likelihood bandwidth selection maximises
    bandwidths                   the list used
  Two calls give the same bits.  ValueError before any device work for what the C ABI refuses."""
  p3 = _sets("kde", points, "points")
  x3 = None if sources is None else _sets("kde", sources, "sources")
  loo = (x3 is None) if loo is None else bool(loo)
  kde_check_shapes((p3 if x3 is None else x3).shape, None if x3 is None else p3.shape, loo)
  if bandwidths is None:
    bandwidths = kde_bandwidths(p3 if x3 is None else x3)
  spec = kde_spec(bandwidths, loo)
  if x3 is None:
    _, one, (p3, _) = _stage(points, p3, p3[:, :0])           # (the device is the points', or the current one)
    log_rho, score, sums = _call(spec, p3, None, want_score)
  else:
    _, one, (p3, x3) = _stage(points, p3, x3)
    log_rho, score, sums = _call(spec, x3, p3, want_score)
  return {"log_density": _unstack(log_rho, one), "score": _unstack(score, one),
          "mean_log_density": _unstack(sums / p3.shape[1], one),
          "bandwidths": [float(spec.bw[i]) for i in range(spec.n_bw)]}
