"""float64 NumPy restatement of the recursion of cnf_sinkhorn (include/cnf_ot_amd.h): log-domain Sinkhorn on the cost
C(x, y) = |x - y|^2 / 2 with uniform weights, four potentials updated simultaneously by averaged steps, one final pass
without averaging; chunked over rows.  The schedule is taken as given: nothing here decides convergence.  A helper: no
tests in it.

  T(h; rows, cols, e)_i = -e log( (1 / n_cols) sum_j exp((h_j - C(row_i, col_j)) / e) )
  k = 0 .. n - 1:  f <- (f + T(g; x, y, e_k)) / 2,  g <- (g + T(f; y, x, e_k)) / 2,
                   p <- (p + T(p; x, x, e_k)) / 2,  q <- (q + T(q; y, y, e_k)) / 2          (all from the old state)
  final, at e_{n-1}:  f* = T(g),  g* = T(f),  p* = T(p),  q* = T(q)
"""
import numpy as np

CHUNK = 512


def schedule(x, y, eps, ratio=0.8, extra=10):
  """The squared diagonal of the joint bounding box times ratio^k while that is > eps, then `extra` entries at eps"""
  pts = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, np.shape(x)[-1]),
                        np.asarray(y, dtype=np.float64).reshape(-1, np.shape(y)[-1])])
  v = float(((pts.max(0) - pts.min(0)) ** 2).sum())
  out = []
  while v > eps:
    out.append(v)
    v *= ratio
  return out + [float(eps)] * extra


def softmin(h, rows, cols, eps, want_plan=False):
  """T(h; rows, cols, eps) [n_rows]; with want_plan also (the barycentric map sum_j w_ij col_j [n_rows, D], the plan's
  row standard deviation sqrt(sum_j w_ij |col_j - map_i|^2) [n_rows], the largest C_ij)"""
  rows, cols, h = (np.asarray(a, dtype=np.float64) for a in (rows, cols, h))
  out = np.empty(len(rows))
  bary = np.empty_like(rows) if want_plan else None
  sigma = np.empty(len(rows)) if want_plan else None
  c_max = 0.0
  c2 = 0.5 * (cols * cols).sum(1)
  for i0 in range(0, len(rows), CHUNK):
    # |r|^2 / 2 + |c|^2 / 2 - r.c: in float64 the cancellation costs 1e-16 |r| |c|, and a product is what keeps the
    # restatement of 2 048 x 1 500 points over 16 iterations at a few seconds
    r = rows[i0:i0 + CHUNK]
    C = np.maximum(0.5 * (r * r).sum(1)[:, None] + c2[None, :] - r @ cols.T, 0.0)
    a = (h[None, :] - C) / eps
    m = a.max(1)
    e = np.exp(a - m[:, None])
    s = e.sum(1)
    out[i0:i0 + CHUNK] = -eps * (m + np.log(s) - np.log(len(cols)))
    if want_plan:
      w = e / s[:, None]
      b = w @ cols
      bary[i0:i0 + CHUNK] = b
      d2 = ((cols[None, :, :] - b[:, None, :]) ** 2).sum(-1)
      sigma[i0:i0 + CHUNK] = np.sqrt((w * d2).sum(1))
      c_max = max(c_max, float(C.max()))
  return (out, bary, sigma, c_max) if want_plan else out


def run(x, y, sched):
  """The recursion on one set.  A dict: f, g, p, q (the final potentials), prev (the four before the final pass), sums
  [6] as cnf_sinkhorn writes them, divergence, ot_xy, map (Txy [N, D]), txx, xgrad [N, D], sigma [N] (the x-y plan's
  row standard deviation), c_max (the largest cost of the four blocks) and h_max (the largest |potential| met)"""
  x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
  N, M = len(x), len(y)
  f, g, p, q = np.zeros(N), np.zeros(M), np.zeros(N), np.zeros(M)
  h_max = 0.0
  for e in sched:
    f, g, p, q = (0.5 * (f + softmin(g, x, y, e)), 0.5 * (g + softmin(f, y, x, e)), 0.5 * (p + softmin(p, x, x, e)),
                  0.5 * (q + softmin(q, y, y, e)))
    h_max = max(h_max, *(float(np.abs(v).max()) for v in (f, g, p, q)))
  e = sched[-1]
  fs, txy, sigma, c_xy = softmin(g, x, y, e, True)
  ps, txx, _, c_xx = softmin(p, x, x, e, True)
  gs = softmin(f, y, x, e)
  qs, _, _, c_yy = softmin(q, y, y, e, True)
  h_max = max(h_max, *(float(np.abs(v).max()) for v in (fs, gs, ps, qs)))
  sums = np.array([fs.sum(), gs.sum(), ps.sum(), qs.sum(), max(np.abs(fs - f).max(), np.abs(gs - g).max()),
                   max(np.abs(ps - p).max(), np.abs(qs - q).max())])
  return {"f": fs, "g": gs, "p": ps, "q": qs, "prev": (f, g, p, q), "sums": sums,
          "divergence": (sums[0] - sums[2]) / N + (sums[1] - sums[3]) / M, "ot_xy": sums[0] / N + sums[1] / M,
          "map": txy, "txx": txx, "xgrad": (txx - txy) / N, "sigma": sigma, "c_max": max(c_xy, c_xx, c_yy), "h_max": h_max}


def clouds(D, N, M, seed, shift=0.3, scale=1.2, S=None):
  """The tests' inputs: x ~ N(0, I), y ~ N(shift (1, ..., 1), scale^2 I), rounded to float32 ([S, ., D] with S)"""
  rng = np.random.default_rng(seed)
  lead = () if S is None else (S,)
  x = rng.standard_normal(lead + (N, D)).astype(np.float32)
  y = (shift + scale * rng.standard_normal(lead + (M, D))).astype(np.float32)
  return x, y
