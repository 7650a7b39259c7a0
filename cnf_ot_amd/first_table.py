"""numpy float64 restatement of the `first` spline's inverse table (cnf_ot_amd/csrc/cnf_first_table.h).

The `first` spline of the flow is one unconditional rational-quadratic spline: its inverse  v -> (g^-1(v),
-log g'(g^-1(v)))  depends on nothing but the parameters.  first_table_kernel tabulates it once per parameter load
and certifies the table against the float64 closed form; the sampling-direction L = 2 table flow kernels then read
it instead of solving the quadratic per sample.  This module states the same construction in numpy so that the tests
can hold the device table to it (tests/test_first_table.py, tests/test_gpu_first_table.py).  Format:

  * FT_CELLS uniform cells over [range_min, range_max]; a cell that holds one interior y knot of the spline is split
    there into two pieces (the spline is only C^1 at a knot): FT_CELLS + K - 1 pieces, in ascending order.
  * a piece's row: the quintic through its six Chebyshev-Lobatto nodes (end points included, so neighbours agree at
    their common edge) of `out` and of `ld`, as coefficients (o0, l0, o1, l1, ..., o5, l5) about `ref`: the cell's
    midpoint, or the knot for the two pieces of a split cell (both rounded to float32: the kernel subtracts that).
  * a cell's grid entry: (ref, next breakpoint or +inf, byte offset of the cell's first row, 0).
  * certified: every piece meets the budget at FT_PROBES interior points, no cell holds two knots, no knot lies within
    edge_guard(lo, hi) of a cell edge (the kernel's fp32 cell index may be off by one there), and everything is finite.
  * in the prepared model buffer the table follows FT_WORDS status words (word 0: FT_CERTIFIED or 0).
"""
import numpy as np

FT_CELLS = 1024
FT_DEG = 5
FT_ROW = 2 * (FT_DEG + 1)          # floats per row
FT_PROBES = 17
FT_BUDGET = 2.4e-7                 # two fp32 ulps at the value's magnitude
FT_WORDS = 4                       # status words in front of the grid
FT_CERTIFIED = 0x31305446
FT_K = 5                           # the table path's bin count: FT_CELLS + FT_K - 1 rows


def edge_guard(lo, hi):
  """Twice the position error of the kernel's fp32 cell index: cs, c0 and the FMA's result are each rounded once,
  2^-24 relative, on magnitudes |v| cs, |lo| cs and the index itself (ft_edge_guard in cnf_first_table.h)."""
  return 2.0 ** -23 * (2.0 * max(abs(lo), abs(hi)) + (hi - lo))


def first_header(params, K=5, lo=-10.0, hi=10.0, min_bin=1e-4, min_slope=1e-4):
  """The float64 header of prepare_kernel: knots and knot slopes of the `first` spline."""
  p = np.asarray(params, dtype=np.float32).astype(np.float64)
  offset = np.log(np.exp(1.0 - min_slope) - 1.0)
  total = (hi - lo) - K * min_bin

  def knots(u):
    e = np.exp(u - u.max())
    s = 0.0
    for k in range(K):
      s += e[k]
    pos = [lo]
    run = 0.0
    for k in range(K - 1):
      run += e[k] / s * total + min_bin
      pos.append(lo + run)
    pos.append(hi)
    return np.array(pos)

  xk, yk = knots(p[:K]), knots(p[K:2 * K])
  v = p[2 * K:3 * K + 1] + offset
  d = np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v))) + min_slope
  return dict(K=K, lo=lo, hi=hi, xk=xk, yk=yk, d=d)


def inverse_closed(h, k, v):
  """(g^-1(v), -log g') of bin k at v, float64 closed form (the flow kernel's root, without its fp32 rounding)."""
  v = np.asarray(v, dtype=np.float64)
  k = np.asarray(k)
  x0, y0 = h["xk"][k], h["yk"][k]
  bw, bh = h["xk"][k + 1] - x0, h["yk"][k + 1] - y0
  s = bh / bw
  d0, d1 = h["d"][k], h["d"][k + 1]
  st = d1 + d0 - 2.0 * s
  dy = v - y0
  c2 = 2.0 * s * dy
  b = d0 * bh - st * dy
  a = s * bh - b
  z = c2 / (b + np.sqrt(b * b + a * (c2 + c2)))
  omz = 1.0 - z
  num2 = d1 * z * z + 2.0 * s * z * omz + d0 * omz * omz
  den = s + st * z * omz
  return x0 + bw * z, -np.log(s * s * num2 / (den * den))


def pieces(h):
  """(a, b, ref, bin) of every piece in order, the cell and half (0 whole, 1 lower, 2 upper) it is, and the
  geometric reasons for refusal."""
  lo, hi, K = h["lo"], h["hi"], h["K"]
  cw = (hi - lo) / FT_CELLS
  yk = h["yk"]
  kc = [int(np.floor((yk[j] - lo) / cw)) for j in range(1, K)]
  ok = True
  guard = edge_guard(lo, hi)
  for j in range(K - 1):
    c = kc[j]
    if j > 0 and kc[j - 1] == c:
      ok = False
    e0, e1 = lo + c * cw, (lo + (c + 1) * cw if c + 1 < FT_CELLS else hi)
    if yk[j + 1] - e0 < guard or e1 - yk[j + 1] < guard:
      ok = False
  out = []
  for p in range(FT_CELLS + K - 1):
    m, half, knot = 0, 0, 0
    for j in range(K - 1):
      q = kc[j] + j
      if q + 1 <= p:
        m += 1
      if p == q + 1:
        half, knot = 2, j + 1
      elif p == q and half == 0:
        half, knot = 1, j + 1
    c = min(max(p - m, 0), FT_CELLS - 1)
    a, b = lo + c * cw, (lo + (c + 1) * cw if c + 1 < FT_CELLS else hi)
    nb = sum(1 for j in range(K - 1) if kc[j] < c)
    if half == 0:
      ref, k = 0.5 * (a + b), nb
    elif half == 1:
      b, ref, k = yk[knot], yk[knot], knot - 1
    else:
      a, ref, k = yk[knot], yk[knot], knot
    out.append((a, b, float(np.float32(ref)), min(k, K - 1), c, half))
  return out, ok, kc


_NODES = np.array([-1.0, -0.8090169943749475, -0.30901699437494745, 0.30901699437494745, 0.8090169943749475, 1.0])
_PROBES = (2.0 * np.arange(FT_PROBES) + 1.0) / FT_PROBES - 1.0


def _monomial(x, f):
  """Coefficients about 0 of the polynomials through (x[p, i], f[p, i]), one per row p: Newton's divided differences,
  then nested multiplication -- the operations of first_table_kernel, in its order."""
  n = x.shape[1]
  c = np.array(f, dtype=np.float64)
  for j in range(1, n):
    for i in range(n - 1, j - 1, -1):
      c[:, i] = (c[:, i] - c[:, i - 1]) / (x[:, i] - x[:, i - j])
  m = np.zeros_like(c)
  m[:, 0] = c[:, n - 1]
  for i in range(n - 2, -1, -1):
    for q in range(n - 1 - i, 0, -1):
      m[:, q] = m[:, q - 1] - x[:, i] * m[:, q]
    m[:, 0] = c[:, i] - x[:, i] * m[:, 0]
  return m


def _horner(co, dv):
  """co [p, n] at dv [p, m], float64 Horner."""
  r = np.zeros_like(dv) + co[:, -1:]
  for q in range(co.shape[1] - 2, -1, -1):
    r = r * dv + co[:, q:q + 1]
  return r


def build(params, probes=_PROBES, **kw):
  """-> dict(rows float32 [pieces, FT_ROW], grid [FT_CELLS, 4] (ref, next breakpoint, row byte offset, 0),
  certified bool, err: the largest budget-relative error met at `probes` (inf: something was not finite),
  piece_err: the same per piece, geom: pieces(), geom_ok, header)."""
  h = first_header(params, **kw)
  ps, ok, kc = pieces(h)
  a, b, ref = (np.array([q[i] for q in ps], dtype=np.float64) for i in range(3))
  k = np.array([q[3] for q in ps])
  mid, rad = 0.5 * (a + b), 0.5 * (b - a)
  rows = np.zeros((len(ps), FT_ROW), dtype=np.float32)
  with np.errstate(all="ignore"):
    xn = mid[:, None] + rad[:, None] * _NODES[None, :]
    xn[:, 0], xn[:, -1] = a, b
    o, l = inverse_closed(h, k[:, None], xn)
    rows[:, 0::2] = _monomial(xn - ref[:, None], o)
    rows[:, 1::2] = _monomial(xn - ref[:, None], l)
    xp = mid[:, None] + rad[:, None] * np.asarray(probes)[None, :]
    o, l = inverse_closed(h, k[:, None], xp)
    eo = np.abs(_horner(rows[:, 0::2].astype(np.float64), xp - ref[:, None]) - o) / np.maximum(1.0, np.abs(o))
    el = np.abs(_horner(rows[:, 1::2].astype(np.float64), xp - ref[:, None]) - l) / np.maximum(1.0, np.abs(l))
    e = np.maximum(eo.max(axis=1), el.max(axis=1))
    e[~(np.isfinite(eo).all(axis=1) & np.isfinite(el).all(axis=1) & np.isfinite(rows).all(axis=1))] = np.inf
  worst = float(e.max())
  grid = np.zeros((FT_CELLS, 4), dtype=np.float64)
  K = h["K"]
  for c in range(FT_CELLS):
    base = c + sum(1 for j in range(K - 1) if kc[j] < c)
    split = any(kc[j] == c for j in range(K - 1))
    grid[c, 0] = ps[base][2]
    grid[c, 1] = ps[base][2] if split else np.inf
    grid[c, 2] = base * FT_ROW * 4
  return dict(rows=rows, grid=grid, certified=bool(ok and worst <= FT_BUDGET), err=worst, piece_err=e, geom=ps,
              geom_ok=ok, header=h)


def evaluate(tab, v):
  """The kernel's lookup in float64 on the float32 table: (out, ld) at v in [lo, hi]."""
  h = tab["header"]
  v = np.asarray(v, dtype=np.float64)
  c = np.clip(np.floor((v - h["lo"]) * (FT_CELLS / (h["hi"] - h["lo"]))).astype(np.int64), 0, FT_CELLS - 1)
  g = tab["grid"][c]
  row = (g[:, 2] / (FT_ROW * 4)).astype(np.int64) + (v >= g[:, 1])
  dv = v - g[:, 0]
  co = tab["rows"][row].astype(np.float64)
  o = co[:, 2 * FT_DEG].copy()
  l = co[:, 2 * FT_DEG + 1].copy()
  for q in range(FT_DEG - 1, -1, -1):
    o = o * dv + co[:, 2 * q]
    l = l * dv + co[:, 2 * q + 1]
  return o, l
