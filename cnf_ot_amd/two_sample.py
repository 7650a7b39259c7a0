"""Distances between two point clouds -- what compares a flow with a target that exists only as samples: the kernel
two-sample statistics (cnf_mmd2) and their permutation test (cnf_mmd_perm), the Sinkhorn divergence (cnf_sinkhorn), the
sliced Wasserstein distance (cnf_sliced_w2) and the nearest-neighbour estimates of entropy and KL (cnf_knn).  The
kernels are five units; what surrounds a call is stated once here: the sets
as [S, N, D] (`_sets`), the shape check (`_check_shapes`), the staging on the device (`_stage`), the workspace
(`_workspace`), the result of a 2-D x (`_unstack`), one call per 64 sets (`_per_64_sets`) and a spec's numbers as
float32 holds them (`_floats32`, `_fits`).  `utils` re-exports the public names.
"""
import math

import numpy as np
import torch

from . import _capi
from .flows import _OnDevice, _stream_ptr


# ---- what the units share ----------------------------------------------------------------------------------------------

def _sets(fn, t, name):
  """A point set, or S of them, as an [S, N, D] tensor where it is ([N, D]: S = 1)."""
  t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
  if t.dim() == 2:
    t = t[None]
  if t.dim() != 3:
    raise ValueError(f"{fn}: {name} must be [N, D] or [S, N, D], not {tuple(t.shape)}")
  return t


def _check_shapes(fn, x_shape, y_shape, lo, hi):
  """ValueError for ([S, N, D], [S, M, D]) outside S in 1..64, N, M in lo..hi (a power of two), D in 1..14."""
  (S, N, D), (Sy, M, Dy) = x_shape, y_shape
  if S != Sy or D != Dy:
    raise ValueError(f"{fn}: x {tuple(x_shape)} and y {tuple(y_shape)} differ in the number of sets or in the dimension")
  if not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or min(N, M) < lo or max(N, M) > hi:
    raise ValueError(f"{fn}: needs 1..{_capi.MMD_MAX_SETS} sets of {lo}..2^{hi.bit_length() - 1} points of dimension "
                     f"1..{_capi.MMD_MAX_DIM}, not x {tuple(x_shape)}, y {tuple(y_shape)}")


def _stage(x, x3, y3, *extras):
  """(device, whether x came in 2-D, [x3, y3, *extras] as the kernels read them): the device is x's if x is on one, else
  y's, else the current one; the tensors detached, float32, contiguous, there."""
  dev = x3.device if x3.is_cuda else (y3.device if y3.is_cuda else torch.device("cuda", torch.cuda.current_device()))
  return dev, np.ndim(x) == 2, [t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in (x3, y3, *extras)]


def _workspace_bytes(query, *args):
  """What the unit's workspace query (its name) answers for `args`."""
  nbytes = _capi.ctypes.c_int64(0)
  _capi.check(getattr(_capi.lib(), query)(*args, _capi.ctypes.byref(nbytes)), query)
  return nbytes.value


_SLICED_WS = {}                                  # device -> the cached workspace (grown, never shrunk)


def _workspace(dev, nbytes, cache=None):
  """A workspace of at least nbytes on dev, as doubles; cache: a dict that keeps one per device, replaced when it is
  too small."""
  new = lambda: torch.empty(-(-nbytes // 8), dtype=torch.float64, device=dev)
  if cache is None:
    return new()
  if cache.get(dev) is None or cache[dev].numel() * 8 < nbytes:
    cache[dev] = None                            # (the old one is released before the new one is asked for)
    cache[dev] = new()
  return cache[dev]


def _unstack(t, one):
  """A per-set result [S, ...] as the caller gets it: set 0 alone where x came in 2-D; None stays None."""
  return t if t is None or not one else t[0]


def _ptr(t):
  return None if t is None else t.data_ptr()


def _per_64_sets(call, *sets):
  """call(*chunks) for every 64 sets of the staged tensors `sets` ([S, ...] each, any S), a tensor or a tuple of tensors
  and Nones: the chunks' results concatenated (up to 64 sets: the one call's result as it is)."""
  step = _capi.MMD_MAX_SETS
  parts = [call(*(t[i:i + step] for t in sets)) for i in range(0, sets[0].shape[0], step)]
  if len(parts) == 1:
    return parts[0]
  if torch.is_tensor(parts[0]):
    return torch.cat(parts)
  return tuple(None if p[0] is None else torch.cat(p) for p in zip(*parts))


_F32_MAX, _F32_MIN = 3.4028234663852886e38, 1.1754943508222875e-38     # float32's largest and smallest normal number


def _fits(v):
  return math.isfinite(v) and abs(v) <= _F32_MAX


def _floats32(v):
  """The numbers of a list, an array or a tensor as Python floats, each rounded to float32 (as the kernel sees them)"""
  return [float(np.float32(b)) for b in np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)]


# ---- kernel two-sample statistics -------------------------------------------------------------------------------------
# The reference: with samples of the target alone KL cannot be computed and "we need to shift to other integral
# probability metric, e.g. MMD" (tests/test_wasserstein_geodesic.py:165-169).  One fused launch over all sets
# (cnf_mmd2); composed in torch the same statistic materialises three N x M matrices.

MEDIAN_BANDWIDTH_FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0)


def median_bandwidths(y, max_rows: int = 1024):
  """The median heuristic: the median pair distance of the first <= 1 024 rows of y ([M, D], or the first set of
  [S, M, D]) times (1/4, 1/2, 1, 2, 4), computed in torch (float64); a list of 5 floats."""
  y = torch.as_tensor(y)
  if y.dim() == 3:
    y = y[0]
  if y.dim() != 2 or y.shape[0] < 2:
    raise ValueError(f"median_bandwidths: expected [M >= 2, D] points, got {tuple(y.shape)}")
  med = float(torch.pdist(y[:max_rows].double()).median())
  if not (med > 0.0 and np.isfinite(med)):
    raise ValueError(f"median_bandwidths: the median pair distance is {med}")
  return [f * med for f in MEDIAN_BANDWIDTH_FACTORS]


def mmd_spec(bandwidths, kind="gaussian"):
  """(CnfMmdSpec, the bandwidths as a list) -- ValueError for what cnf_mmd2 refuses in a spec."""
  if kind not in _capi.MMD_KINDS:
    raise ValueError(f"mmd2: kind is 'gaussian' or 'energy', not {kind!r}")
  spec = _capi.CnfMmdSpec()
  spec.kind = _capi.MMD_KINDS[kind]
  if kind == "energy":
    return spec, []
  bws = [float(b) for b in np.asarray(bandwidths.cpu() if torch.is_tensor(bandwidths) else bandwidths,
                                      dtype=np.float64).reshape(-1)]
  if not 1 <= len(bws) <= _capi.MMD_MAX_BW:
    raise ValueError(f"mmd2: between 1 and {_capi.MMD_MAX_BW} bandwidths, not {len(bws)}")
  for b in bws:
    b32 = float(np.float32(b))      # (as the kernel sees it; 1 / bw^2 must stay in float32's range)
    if not (b32 > 0.0 and np.isfinite(b32) and 1.0 / (b32 * b32) <= 3.0e38):
      raise ValueError(f"mmd2: every bandwidth must be positive and finite (in float32, with 1 / bw^2): {bws}")
  spec.n_bw = len(bws)
  for i, b in enumerate(bws):
    spec.bw[i] = b
  return spec, [float(spec.bw[i]) for i in range(len(bws))]


def mmd_check_shapes(x_shape, y_shape):
  """ValueError for sets cnf_mmd2 refuses: ([S, N, D], [S, M, D]) with S in 1..64, N, M >= 2, D in 1..14."""
  _check_shapes("mmd2", x_shape, y_shape, 2, 1 << 24)


def mmd2_from_sums(sums, N, M):
  """The unbiased MMD^2 [S] from raw sums [S, 3] = (sxx, syy, sxy)."""
  return sums[:, 0] / (N * (N - 1.0)) + sums[:, 1] / (M * (M - 1.0)) - 2.0 * sums[:, 2] / (float(N) * M)


def mmd2(x, y, bandwidths=None, kind="gaussian", want_grad=False) -> dict:
  """The unbiased kernel two-sample statistic between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D]
  (set s of x against set s of y), ONE fused launch over all sets and all three pair blocks (cnf_mmd2):
    kind="gaussian": k(x, y) = sum_b exp(-|x - y|^2 / (2 bw_b^2)) over up to 8 `bandwidths` (None:
                     median_bandwidths(y)) -- MMD^2
    kind="energy":   k(x, y) = -|x - y| -- the energy distance 2 E|x - y| - E|x - x'| - E|y - y'|
  float32 on the device (float64 inputs are rounded; host inputs are uploaded).  Returns a dict: mmd2 [S] (float64),
  sums [S, 3] (the raw sxx, syy, sxy: diagonal left out), bandwidths (a list; empty for energy) and, with want_grad,
  grad [S, N, D] (float32; [N, D] for 2-D x) = d mmd2 / d x.  Two calls give the same bits.  ValueError before any
  device work for what the C ABI refuses (D outside 1..14, N or M < 2, more than 64 sets or 8 bandwidths, a bandwidth
  that is not positive and finite, an unknown kind) and for x and y that differ in S or D."""
  x3, y3 = _sets("mmd2", x, "x"), _sets("mmd2", y, "y")
  mmd_check_shapes(x3.shape, y3.shape)
  if kind == "gaussian" and bandwidths is None:
    bandwidths = median_bandwidths(y3)
  spec, bws = mmd_spec(bandwidths, kind)
  S, N, D = x3.shape
  M = y3.shape[1]
  dev, one, (x3, y3) = _stage(x, x3, y3)
  ws = _workspace(dev, _workspace_bytes("cnf_mmd_workspace", S, N, M, D, 1 if want_grad else 0))
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_mmd2(_capi.ctypes.byref(spec), S, x3.data_ptr(), N, y3.data_ptr(), M, D, sums.data_ptr(),
                                     _ptr(grad), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)), "cnf_mmd2")
  out = {"mmd2": mmd2_from_sums(sums, N, M), "sums": sums, "bandwidths": bws}
  if want_grad:
    out["grad"] = _unstack(grad, one)
  return out


# ---- the permutation test of the kernel two-sample statistics: a value of MMD^2 as a p-value --------------------------
# The statistic is recomputed under relabellings of the pooled sample and the observed value is ranked among them.  One
# cnf_mmd_perm call forms every pair kernel value once and uses it for all label vectors, on the
# matrix cores; as calls of mmd2 on shuffled copies the same test evaluates every pair value once per vector.

PERM_MIN_VECTORS, PERM_MAX_VECTORS, PERM_MAX_POINTS = 32, 1024, 1 << 20


def permutation_labels(N, M, n_perm, seed=0):
  """The label words of a permutation test of N against M points, an int32 CPU tensor [N + M, (n_perm + 1) / 32]: bit b
  of word w of pooled point j (j < N: x_j, else y_{j - N}) is set where j belongs to the first sample under label
  vector 32 w + b.  Vector 0 is the identity labelling (the first N points); vectors 1..n_perm are uniform random
  subsets of size N, drawn by numpy's default_rng(seed) -- a fixed function of (N, M, n_perm, seed).  ValueError unless
  n_perm + 1 is a multiple of 32 within 32..1024 and N, M >= 1."""
  N, M, P = int(N), int(M), int(n_perm) + 1
  if P % 32 or not PERM_MIN_VECTORS <= P <= PERM_MAX_VECTORS:
    raise ValueError(f"permutation_labels: n_perm + 1 must be a multiple of 32 within {PERM_MIN_VECTORS}.."
                     f"{PERM_MAX_VECTORS}, not {P}")
  if N < 1 or M < 1:
    raise ValueError(f"permutation_labels: needs N, M >= 1, not {N}, {M}")
  rng = np.random.default_rng(int(seed))
  member = np.zeros((N + M, P), dtype=bool)
  member[:N, 0] = True
  for p in range(1, P):
    member[rng.choice(N + M, size=N, replace=False, shuffle=False), p] = True
  return pack_labels(member)


def pack_labels(member):
  """Label words [n, P / 32] (int32 CPU tensor) of a membership matrix [n, P] (True: first sample), P a multiple of 32"""
  member = np.asarray(member, dtype=bool)
  n, P = member.shape
  if P % 32:
    raise ValueError(f"pack_labels: the number of label vectors must be a multiple of 32, not {P}")
  words = (member.reshape(n, P // 32, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
  return torch.from_numpy(words.view(np.int32).copy())


def mmd_perm_check_shapes(x_shape, y_shape, labels_shape=None):
  """ValueError for what cnf_mmd_perm refuses: ([S, N, D], [S, M, D], [N + M, W]) with S in 1..64, N, M >= 2, N + M <=
  2^20, D in 1..14 and W = P / 32 words in 1..32."""
  _check_shapes("mmd_perm", x_shape, y_shape, 2, PERM_MAX_POINTS)
  n = x_shape[1] + y_shape[1]
  if n > PERM_MAX_POINTS:
    raise ValueError(f"mmd_perm: the pooled sample has at most 2^20 points, not {n}")
  if labels_shape is not None and (len(labels_shape) != 2 or labels_shape[0] != n
                                   or not 1 <= labels_shape[1] <= PERM_MAX_VECTORS // 32):
    raise ValueError(f"mmd_perm: labels must be [{n}, P / 32] words with P in {PERM_MIN_VECTORS}..{PERM_MAX_VECTORS}, not "
                     f"{tuple(labels_shape)}")


def permutation_p_value(observed, null):
  """(1 + #{null >= observed}) / (1 + n_perm) for observed [S] and null [S, n_perm]: the usual estimate, never 0; a
  tie counts."""
  return (1.0 + (null >= observed[:, None]).sum(1).double()) / (1.0 + null.shape[1])


def mmd_permutation_test(x, y, bandwidths=None, kind="gaussian", n_perm=255, seed=0, labels=None) -> dict:
  """The permutation test of the unbiased kernel two-sample statistic between the point sets x [N, D] or [S, N, D] and
  y [M, D] or [S, M, D] (set s of x against set s of y; kind and bandwidths as `mmd2`, None: median_bandwidths(y)): the
  statistic under n_perm relabellings of the pooled sample, ONE cnf_mmd_perm call per 64 sets.  labels: the label words
  [N + M, P / 32] (None: permutation_labels(N, M, n_perm, seed)); with labels given, n_perm = P - 1 and vector 0 is
  taken as the observed labelling.  The same label vectors serve all sets.  float32 on the device.  Returns a dict:
    mmd2 [S]          label vector 0's statistic (float64)
    null [S, n_perm]  the statistic under vectors 1..n_perm
    p_value [S]       (1 + #{null >= mmd2}) / (1 + n_perm)
    counts [P]        the first sample's size under every vector (int64, CPU)
    bandwidths        a list; empty for energy
    raw               {"q": [S, P], "r": [S, P], "t": [S]}: s' K s, 1' K s and 1' K 1 of the pooled zero-diagonal kernel
                      matrix, from which every value can be audited
  Evaluation only: no gradient.  Two calls give the same bits.  ValueError before any device work for what the C ABI
  refuses and for x, y and labels that do not fit together."""
  x3, y3 = _sets("mmd_perm", x, "x"), _sets("mmd_perm", y, "y")
  (S, N, D), M = x3.shape, y3.shape[1]
  if S != y3.shape[0]:
    raise ValueError(f"mmd_perm: x {tuple(x3.shape)} and y {tuple(y3.shape)} differ in the number of sets")
  one_call = [(min(S, _capi.MMD_MAX_SETS),) + tuple(t.shape[1:]) for t in (x3, y3)]      # (any S: 64 sets per call)
  mmd_perm_check_shapes(*one_call)
  if labels is None:
    labels = permutation_labels(N, M, n_perm, seed)
  labels = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))
  mmd_perm_check_shapes(*one_call, tuple(labels.shape))
  if labels.dtype != torch.int32:
    raise ValueError(f"mmd_perm: labels are int32 words, not {labels.dtype}")
  P = 32 * labels.shape[1]
  if kind == "gaussian" and bandwidths is None:
    bandwidths = median_bandwidths(y3)
  spec, bws = mmd_spec(bandwidths, kind)
  dev, one, (x3, y3) = _stage(x, x3, y3)
  words = labels.detach().to(device=dev).contiguous()

  def call(xc, yc):
    Sc = xc.shape[0]
    ws = _workspace(dev, _workspace_bytes("cnf_mmd_perm_workspace", Sc, N, M, D, P))
    stats = torch.empty(Sc, P, dtype=torch.float64, device=dev)
    raw = torch.empty(Sc * (2 * P + 1), dtype=torch.float64, device=dev)
    with _OnDevice(dev):
      _capi.check(_capi.lib().cnf_mmd_perm(_capi.ctypes.byref(spec), Sc, xc.data_ptr(), N, yc.data_ptr(), M, D,
                                           words.data_ptr(), P, stats.data_ptr(), raw.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 8, _stream_ptr(dev)), "cnf_mmd_perm")
    return stats, raw[:Sc * 2 * P].view(Sc, P, 2), raw[Sc * 2 * P:]

  stats, qr, t = _per_64_sets(call, x3, y3)
  bits = (labels.cpu().numpy().view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
  return {"mmd2": stats[:, 0], "null": stats[:, 1:], "p_value": permutation_p_value(stats[:, 0], stats[:, 1:]),
          "counts": torch.from_numpy(bits.reshape(N + M, P).sum(0, dtype=np.int64)), "bandwidths": bws,
          "raw": {"q": qr[..., 0], "r": qr[..., 1], "t": t}}


# ---- the Sinkhorn divergence: an optimal-transport estimate between point clouds, in transport units -----------------
# Log-domain Sinkhorn on C(x, y) = |x - y|^2 / 2, debiased: S_eps(x, y) = OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2,
# with the dual potentials, the barycentric map (an estimate of the Monge map) and the gradient in x.  The iteration
# count and the eps of every iteration are inputs of the kernel (cnf_sinkhorn): the schedule below is
# the usual annealing, and `change` in the result says how far from its fixed point the recursion stopped.

SINKHORN_MAX_ITERS, SINKHORN_MAX_POINTS = 512, 1 << 20


def sinkhorn_check_shapes(x_shape, y_shape):
  """ValueError for sets cnf_sinkhorn refuses: ([S, N, D], [S, M, D]) with S in 1..64, N, M in 2..2^20, D in 1..14."""
  _check_shapes("sinkhorn", x_shape, y_shape, 2, SINKHORN_MAX_POINTS)


def sinkhorn_check_schedule(schedule):
  """The schedule as a list of floats -- ValueError for what cnf_sinkhorn refuses in one: no entry or more than 512, an
  eps that is not positive and finite or whose inverse leaves float32's range."""
  eps = [float(e) for e in np.asarray(schedule.cpu() if torch.is_tensor(schedule) else schedule, dtype=np.float64).reshape(-1)]
  if not 1 <= len(eps) <= SINKHORN_MAX_ITERS:
    raise ValueError(f"sinkhorn: a schedule has 1..{SINKHORN_MAX_ITERS} entries, not {len(eps)}")
  for e in eps:
    if not (e > 0.0 and np.isfinite(e) and 1.2e-38 <= 1.0 / e <= 2.0e38):
      raise ValueError(f"sinkhorn: every eps must be positive and finite, with 1 / eps in float32's range: {e}")
  return eps


def sinkhorn_schedule(x, y, eps, ratio=0.8, extra=10):
  """The annealing schedule of `sinkhorn`, a list of floats: the squared diagonal of the joint bounding box of x and y
  (all sets), times ratio^k for k = 0, 1, ... while that is > eps, then `extra` entries at eps.  ValueError for an eps
  that is not positive and finite, a ratio outside (0, 1), extra < 0, an empty schedule or more than 512 entries."""
  eps, ratio, extra = float(eps), float(ratio), int(extra)
  if not (eps > 0.0 and np.isfinite(eps)) or not 0.0 < ratio < 1.0 or extra < 0:
    raise ValueError(f"sinkhorn_schedule: needs eps > 0, 0 < ratio < 1 and extra >= 0, not {eps}, {ratio}, {extra}")
  pts = [t.detach().reshape(-1, t.shape[-1]).double() for t in (_sets("sinkhorn", x, "x"), _sets("sinkhorn", y, "y"))]
  lo = torch.minimum(pts[0].min(0).values.cpu(), pts[1].min(0).values.cpu())
  hi = torch.maximum(pts[0].max(0).values.cpu(), pts[1].max(0).values.cpu())
  v = float(((hi - lo) ** 2).sum())
  if not np.isfinite(v):
    raise ValueError("sinkhorn_schedule: the points are not finite")
  out = []
  while v > eps and len(out) + extra <= SINKHORN_MAX_ITERS:
    out.append(v)
    v *= ratio
  out += [eps] * extra
  if len(out) > SINKHORN_MAX_ITERS:
    raise ValueError(f"sinkhorn_schedule: more than {SINKHORN_MAX_ITERS} iterations (diagonal^2 {out[0]:.3g}, eps {eps}, "
                     f"ratio {ratio}, extra {extra})")
  if not out:
    raise ValueError("sinkhorn_schedule: an empty schedule (the bounding box is within eps and extra = 0)")
  return out


def sinkhorn(x, y, eps=0.05, schedule=None, want_grad=False, want_map=False, want_potentials=False) -> dict:
  """The Sinkhorn divergence S_eps between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D] (set s of x
  against set s of y; uniform weights, cost |x - y|^2 / 2), ONE cnf_sinkhorn call over all sets: len(schedule)
  averaged Jacobi iterations of the four potentials f, g (x against y), p (x against x), q (y against y) and a final
  pass at the last eps (the recursion: include/cnf_ot_amd.h).  schedule: the eps of every iteration (None:
  sinkhorn_schedule(x, y, eps); with a schedule `eps` is not used).  float32 on the device (float64 inputs are rounded;
  host inputs are uploaded).  Returns a dict:
    divergence [S]  (sum f* - sum p*) / N + (sum g* - sum q*) / M (float64): an estimate of W2^2 / 2
    ot_xy [S]       sum f* / N + sum g* / M, the entropic cost of x against y alone
    change [S, 2]   the largest |f* - f|, |g* - g| and |p* - p|, |q* - q| of the final pass: 0 at the fixed point
    grad            want_grad: [S, N, D] float32 ([N, D] for 2-D x), the envelope gradient of the divergence in x (the
                    potentials held fixed: exact at the fixed point); else None
    map             want_map: the barycentric map T(x_i) = sum_j pi_ij y_j / sum_j pi_ij, shaped like grad; else None
    f, g, p, q      want_potentials: [S, N], [S, M], [S, N], [S, M] float32; else None
    schedule        the list of eps used
  Two calls give the same bits, and the numbers do not depend on the want_ flags.  ValueError before any device work
  for what the C ABI refuses and for x and y that differ in S or D."""
  x3, y3 = _sets("sinkhorn", x, "x"), _sets("sinkhorn", y, "y")
  sinkhorn_check_shapes(x3.shape, y3.shape)
  sched = sinkhorn_check_schedule(sinkhorn_schedule(x3, y3, eps) if schedule is None else schedule)
  S, N, D = x3.shape
  M = y3.shape[1]
  dev, one, (x3, y3) = _stage(x, x3, y3)
  ws = _workspace(dev, _workspace_bytes("cnf_sinkhorn_workspace", S, N, M, D))
  sums = torch.empty(S, 6, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  tmap = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_map else None
  pot = torch.empty(S, 2 * (N + M), dtype=torch.float32, device=dev) if want_potentials else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_sinkhorn(S, x3.data_ptr(), N, y3.data_ptr(), M, D,
                                         (_capi.ctypes.c_double * len(sched))(*sched), len(sched), sums.data_ptr(),
                                         _ptr(pot), _ptr(grad), _ptr(tmap), ws.data_ptr(), ws.numel() * 8,
                                         _stream_ptr(dev)), "cnf_sinkhorn")
  f, g, p, q = (None,) * 4 if pot is None else pot.split([N, M, N, M], dim=1)
  return {"divergence": (sums[:, 0] - sums[:, 2]) / N + (sums[:, 1] - sums[:, 3]) / M,
          "ot_xy": sums[:, 0] / N + sums[:, 1] / M, "change": sums[:, 4:6], "grad": _unstack(grad, one),
          "map": _unstack(tmap, one), "f": f, "g": g, "p": p, "q": q, "schedule": sched}


# ---- the sliced Wasserstein distance: transport units between point clouds of any size, N log N per projection -------
# Both clouds are projected on P directions; along a direction optimal transport is exact and is a sort.  No eps, no
# iteration count, no debiasing; cost |.|^2 / 2 as `sinkhorn`, so for unit directions drawn uniformly SW <= W2^2 / (2 D),
# and with the coordinate axes as directions sqrt(2 w) is the exact W2 of every marginal (cnf_sliced_w2).

SLICED_MAX_PROJ, SLICED_MAX_POINTS, SLICED_WORKSPACE_BYTES = 1024, 1 << 20, 1 << 30


def sliced_directions(D, P, seed=0, kind="random"):
  """Directions for `sliced_wasserstein`, [P, D] float32 on the host.  kind="random": P unit vectors, Gaussian draws of
  numpy's default_rng(seed) normalised in float64 -- a fixed function of (D, P, seed); for D = 1 the single direction
  +1 (P must be 1: the other direction, -1, gives the same value).  kind="axes": the D coordinate axes (P must be D).
  ValueError for D outside 1..14, P outside 1..1024, an unknown kind or a P the kind does not allow."""
  D, P = int(D), int(P)
  if not 1 <= D <= _capi.MMD_MAX_DIM or not 1 <= P <= SLICED_MAX_PROJ:
    raise ValueError(f"sliced_directions: needs D in 1..{_capi.MMD_MAX_DIM} and P in 1..{SLICED_MAX_PROJ}, not {D}, {P}")
  if kind == "axes":
    if P != D:
      raise ValueError(f"sliced_directions: the axes of dimension {D} are {D} directions, not {P}")
    return torch.eye(D, dtype=torch.float32)
  if kind != "random":
    raise ValueError(f"sliced_directions: kind is 'random' or 'axes', not {kind!r}")
  if D == 1:
    if P != 1:
      raise ValueError(f"sliced_directions: dimension 1 has the single direction +1, not {P}")
    return torch.ones(1, 1, dtype=torch.float32)
  g = np.random.default_rng(int(seed)).standard_normal((P, D))
  return torch.from_numpy((g / np.sqrt((g * g).sum(1, keepdims=True))).astype(np.float32))


def sliced_check_shapes(x_shape, y_shape, theta_shape=None):
  """ValueError for what cnf_sliced_w2 refuses: ([S, N, D], [S, M, D], [P, D]) with S in 1..64, N, M in 1..2^20, D in
  1..14, P in 1..1024."""
  _check_shapes("sliced", x_shape, y_shape, 1, SLICED_MAX_POINTS)
  D = x_shape[2]
  if theta_shape is not None and (len(theta_shape) != 2 or theta_shape[1] != D or not 1 <= theta_shape[0] <= SLICED_MAX_PROJ):
    raise ValueError(f"sliced: directions must be [P, {D}] with P in 1..{SLICED_MAX_PROJ}, not {tuple(theta_shape)}")


def sliced_group(S, N, M, D, P, want_grad, limit=SLICED_WORKSPACE_BYTES):
  """(G, bytes): the largest group of projections whose workspace (cnf_sliced_workspace) is at most `limit` bytes -- 1
  if even that is more -- and that workspace's size.  The size is linear in G, so two calls settle it."""
  size = lambda G: _workspace_bytes("cnf_sliced_workspace", S, N, M, D, G, int(want_grad))
  b1 = size(1)
  G = 1 if P == 1 or b1 >= limit else max(1, min(P, 1 + (limit - b1) // (size(2) - b1)))
  return G, size(G)


def sliced_wasserstein(x, y, directions=None, n_proj=64, seed=0, want_grad=False) -> dict:
  """The sliced Wasserstein distance between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D] (set s of x
  against set s of y; uniform weights, cost |.|^2 / 2), ONE cnf_sliced_w2 call over all sets.  directions: [P, D]
  (None: sliced_directions(D, n_proj, seed), or the single direction of D = 1); they are used as given, not
  normalised.  float32 on the device (float64 inputs are rounded; host inputs are uploaded).  Returns a dict:
    sw [S]               the mean over the directions of the one-dimensional transport cost (float64)
    per_projection [S, P]  that cost per direction: the quantile-function integral, exact for any N and M
    max_sliced [S]       its maximum over the given directions
    directions [P, D]    the directions used, float32 on the device
    grad                 want_grad: [S, N, D] float32 ([N, D] for 2-D x), the envelope gradient of sw in x (the sorting
                         permutations held fixed: exact wherever the projected samples are distinct); else None
  The projections are processed in the largest groups whose workspace stays within 1 GiB (sliced_group); the result
  does not depend on the grouping, and two calls give the same bits.  The workspace is cached per device.  ValueError
  before any device work for what the C ABI refuses and for x, y and directions that differ in S or D."""
  x3, y3 = _sets("sliced", x, "x"), _sets("sliced", y, "y")
  sliced_check_shapes(x3.shape, y3.shape)
  S, N, D = x3.shape
  M = y3.shape[1]
  if directions is None:
    directions = sliced_directions(D, 1 if D == 1 else n_proj, seed)
  th = directions if torch.is_tensor(directions) else torch.as_tensor(np.asarray(directions))
  sliced_check_shapes(x3.shape, y3.shape, tuple(th.shape))
  P = th.shape[0]
  dev, one, (x3, y3, th) = _stage(x, x3, y3, th)
  G, nbytes = sliced_group(S, N, M, D, P, want_grad)
  ws = _workspace(dev, nbytes, cache=_SLICED_WS)
  sums = torch.empty(S, P + 2, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_sliced_w2(S, x3.data_ptr(), N, y3.data_ptr(), M, D, th.data_ptr(), P, G, sums.data_ptr(),
                                          _ptr(grad), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)), "cnf_sliced_w2")
  return {"sw": sums[:, P], "per_projection": sums[:, :P], "max_sliced": sums[:, P + 1], "directions": th,
          "grad": _unstack(grad, one)}


# ---- nearest-neighbour estimates: entropy, cross entropy and KL in nats between point clouds -------------------------
# The note quoted above holds for the plug-in formula; the nearest-neighbour estimators need samples alone.  One fused
# call scans x against x and x against y over all sets (cnf_knn); composed in torch (cdist + topk) the
# same scan materialises the N x M matrix.  No gradient and no training term: the estimator's gradient is too noisy to
# train on, and no reference call site asks for one.

KNN_MAX_K, KNN_MAX_POINTS = _capi.KNN_MAX_K, _capi.KNN_MAX_POINTS


def knn_check_shapes(x_shape, y_shape=None, k=4):
  """ValueError for what cnf_knn refuses: ([S, N, D], [S, M, D] or None, k) with S in 1..64, D in 1..14, k in 1..16, N in
  k + 1..2^20, M in k..2^20."""
  k = int(k)
  if not 1 <= k <= KNN_MAX_K:
    raise ValueError(f"knn: k must be in 1..{KNN_MAX_K}, not {k}")
  _check_shapes("knn", x_shape, x_shape if y_shape is None else y_shape, k, KNN_MAX_POINTS)
  if x_shape[1] < k + 1:
    raise ValueError(f"knn: x needs at least k + 1 = {k + 1} points (a point is not its own neighbour), not {x_shape[1]}")


def knn(x, y=None, k=4, want_indices=False) -> dict:
  """The k nearest neighbours of every point of x [N, D] or [S, N, D] among the OTHER points of x and, with y [M, D] or
  [S, M, D], among the points of y (set s of x against set s of y), ONE cnf_knn call over all sets.  Neighbours are
  ascending by (squared distance as computed in float32 from coordinate differences, index): of two equal distances
  the smaller index comes first, and a duplicate point at another index is a neighbour at distance 0.  float32 on the
  device (float64 inputs are rounded; host inputs are uploaded).  Returns a dict:
    dist_xx, dist_xy  [S, N, k] float32 ([N, k] for 2-D x), ranks 1..k; dist_xy is None without y
    idx_xx, idx_xy    want_indices: the neighbours' rows, int32, shaped like the distances (idx_xy None without y)
    sums              [S, 2, k, 2] float64: per block (self, cross) and rank, the sum of log dist over the rows whose
                      dist is > 0 and the number of rows whose dist is 0 (the cross half: zeros without y) -- what
                      knn_estimates reads
  Rank j does not depend on k, two calls give the same bits, and the numbers do not depend on want_indices.  There is
  no gradient: the estimators built on these distances are for evaluation, their gradient is too noisy to train on.
  ValueError before any device work for what the C ABI refuses and for x and y that differ in S or D."""
  x3 = _sets("knn", x, "x")
  y3 = None if y is None else _sets("knn", y, "y")
  knn_check_shapes(x3.shape, None if y3 is None else y3.shape, k)
  k = int(k)
  S, N, D = x3.shape
  M = 0 if y3 is None else y3.shape[1]
  dev, one, (x3, ys) = _stage(x, x3, x3 if y3 is None else y3)
  y3 = None if y3 is None else ys
  ws = _workspace(dev, _workspace_bytes("cnf_knn_workspace", S, N, M, D, k))
  sums = torch.empty(S, 2, k, 2, dtype=torch.float64, device=dev)
  new = lambda dtype: torch.empty(S, N, k, dtype=dtype, device=dev)
  dxx, dxy = new(torch.float32), None if y3 is None else new(torch.float32)
  ixx = new(torch.int32) if want_indices else None
  ixy = new(torch.int32) if want_indices and y3 is not None else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_knn(S, x3.data_ptr(), N, _ptr(y3), M, D, k, _ptr(dxx), _ptr(ixx), _ptr(dxy), _ptr(ixy),
                                    sums.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)), "cnf_knn")
  out = {"dist_xx": _unstack(dxx, one), "dist_xy": _unstack(dxy, one), "sums": sums}
  if want_indices:
    out.update(idx_xx=_unstack(ixx, one), idx_xy=_unstack(ixy, one))
  return out


def knn_estimates(sums, N, M, D) -> dict:
  """The nearest-neighbour estimators, in nats and in float64, for every rank j = 1..k of sums [S, 2, k, 2] (knn's): with
  psi the digamma function, log V_D = (D / 2) log pi - lgamma(D / 2 + 1) the log volume of the unit ball, and the means
  taken over the rows whose distance is not 0 (sums[..., 0] / (N - sums[..., 1])),
    entropy [S, k]        psi(N) - psi(j) + log V_D + D mean_i log rho_j(i)   (Kozachenko-Leonenko)
    cross_entropy [S, k]  log M  - psi(j) + log V_D + D mean_i log nu_j(i)    (Leonenko-Pronzato-Savani)
    kl [S, k]             cross_entropy - entropy                              (Wang-Kulkarni-Verdu, psi-corrected)
    zeros [S, 2, k]       the rows left out of each mean
  rho_j(i): the distance from x_i to its j-th nearest other point of x; nu_j(i): to its j-th nearest point of the M
  points of y.  M = 0 (no y): cross_entropy and kl are None.  This is the one place the estimators are written down."""
  sums = torch.as_tensor(sums).double()
  k, N, M, D = sums.shape[2], int(N), int(M), int(D)
  psi = lambda v: torch.special.digamma(torch.as_tensor(v, dtype=torch.float64, device=sums.device))
  psi_j = psi(list(range(1, k + 1)))
  log_vd = 0.5 * D * float(np.log(np.pi)) - float(torch.lgamma(torch.tensor(0.5 * D + 1.0, dtype=torch.float64)))
  zeros = sums[..., 1]
  mean = sums[..., 0] / (N - zeros)
  entropy = psi(float(N)) - psi_j + log_vd + D * mean[:, 0]
  cross = None if M == 0 else float(np.log(M)) - psi_j + log_vd + D * mean[:, 1]
  return {"entropy": entropy, "cross_entropy": cross, "kl": None if M == 0 else cross - entropy, "zeros": zeros}


def knn_divergence(x, y, k=4) -> dict:
  """KL(x || y) in nats between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D] from their samples alone
  (knn, knn_estimates): kl, entropy (of x) and cross_entropy [S] (float64) at rank k, by_rank (knn_estimates' dict, every
  rank 1..k), zeros [S, 2, k] and k.  The estimate carries a bias that grows with the dimension: read it beside the same
  estimate between two samples of one law.  No gradient (see knn)."""
  x3, y3 = _sets("knn", x, "x"), _sets("knn", y, "y")
  est = knn_estimates(knn(x3, y3, k)["sums"], x3.shape[1], y3.shape[1], x3.shape[2])
  return {"kl": est["kl"][:, -1], "entropy": est["entropy"][:, -1], "cross_entropy": est["cross_entropy"][:, -1],
          "by_rank": est, "zeros": est["zeros"], "k": int(k)}


def knn_entropy(x, k=4) -> dict:
  """The Kozachenko-Leonenko entropy, in nats, of the point sets x [N, D] or [S, N, D] (the self block of knn alone):
  entropy [S] (float64) at rank k, by_rank, zeros [S, 2, k] and k."""
  x3 = _sets("knn", x, "x")
  est = knn_estimates(knn(x3, None, k)["sums"], x3.shape[1], 0, x3.shape[2])
  return {"entropy": est["entropy"][:, -1], "by_rank": est, "zeros": est["zeros"], "k": int(k)}
