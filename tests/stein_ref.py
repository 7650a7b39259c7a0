"""The kernel Stein discrepancy restated in NumPy: float64 is the reference of tests/test_gpu_stein.py and
tests/test_stein_cpu.py, and the same composition in float32 (pair matrices in float32, reduced in float64) gives the
e_composed of the project's bar  e_fused <= 2 e_composed + 4 EPS scale.

Base kernel k(x, y) = phi(q), q = |d|^2, d = x - y; p0 .. p3 = phi and its first three derivatives in q:
  k_p(x, y) = p0 (s_x . s_y) + 2 p1 d . (s_y - s_x) - 4 p2 q - 2 D p1,     k_p(x, x) = p0(0) |s_x|^2 - 2 D p1(0)
  sums = (sum_{i != j} k_p, sum_i k_p(x_i, x_i)),   rows_i = sum_{j != i} k_p / (N - 1)
  KSD^2_U = sums[0] / (N (N - 1)),   KSD^2_V = (sums[0] + sums[1]) / N^2
  d KSD^2_U / d s_i = 2 / (N (N - 1)) sum_{j != i} (p0 s_j - 2 p1 d)
  d KSD^2_U / d x_i = 2 / (N (N - 1)) sum_{j != i} ((2 p1 s_i . s_j + 4 p2 d . (s_j - s_i) - 8 p3 q - (8 + 4 D) p2) d
                                                    + 2 p1 (s_j - s_i))
  direction_i = mean_j (k s_j + grad_{x_j} k) = ((N - 1) / 2) d KSD^2_U / d s_i + p0(0) s_i / N
"""
import numpy as np


def spec(kind, bws, weights=None, beta=-0.5):
  bws = [float(np.float32(b)) for b in bws]      # (as the kernel receives them)
  ws = [1.0] * len(bws) if weights is None else [float(np.float32(w)) for w in weights]
  return {"kind": kind, "bw": bws, "w": ws, "beta": float(np.float32(beta))}


def kwargs(sp):
  return {"kind": sp["kind"], "bandwidths": sp["bw"], "weights": sp["w"], "beta": sp["beta"]}


def phis(q, sp, dtype=np.float64):
  """(p0, p1, p2, p3) at the squared distances q, in dtype"""
  q = np.asarray(q, dtype=dtype)
  out = [np.zeros_like(q) for _ in range(4)]
  for w, bw in zip(sp["w"], sp["bw"]):
    w, bw = dtype(w), dtype(bw)
    if sp["kind"] == "imq":
      be = dtype(sp["beta"])
      u = q + bw * bw
      t = w * u ** be
      cs = [dtype(1.0), be, be * (be - dtype(1.0)), be * (be - dtype(1.0)) * (be - dtype(2.0))]
      for m in range(4):
        out[m] = out[m] + cs[m] * t / u ** dtype(m)
    else:
      ib = dtype(1.0) / (dtype(2.0) * bw * bw)
      e = w * np.exp(-q * ib)
      for m in range(4):
        out[m] = out[m] + (-ib) ** dtype(m) * e
  return out


def cloud(D, N, seed, scale=1.0, S=None):
  rng = np.random.default_rng(seed)
  shape = (N, D) if S is None else (S, N, D)
  return (scale * rng.standard_normal(shape)).astype(np.float32)


def stats(x, s, sp, dtype=np.float64, chunk=256):
  """Everything cnf_stein and utils.ksd return for ONE set x [N, D] with scores s [N, D], and the scales of the bar: a
  dict of sums (2,), rows [N], grad_x, grad_s, direction [N, D] (float64 arrays; the pair quantities formed in dtype),
  scale_v, scale_gx, scale_gs = the largest per-pair sum of the absolute values of the summands (the gradients' per
  component).  Rows are chunked so that no N x N x D array is held."""
  x, s = np.asarray(x, dtype=dtype), np.asarray(s, dtype=dtype)
  N, D = x.shape
  rows = np.zeros(N)
  gx, gs = np.zeros((N, D)), np.zeros((N, D))
  scale_v = scale_gx = scale_gs = 0.0
  two, four, eight = dtype(2.0), dtype(4.0), dtype(8.0)
  for i0 in range(0, N, chunk):
    xi, si = x[i0:i0 + chunk], s[i0:i0 + chunk]
    d = xi[:, None, :] - x[None, :, :]
    ds = s[None, :, :] - si[:, None, :]
    q = (d * d).sum(-1)
    ss = (si[:, None, :] * s[None, :, :]).sum(-1)
    dds = (d * ds).sum(-1)
    p0, p1, p2, p3 = phis(q, sp, dtype)
    off = np.ones_like(q)
    k = np.arange(len(xi))
    off[k, i0 + k] = 0                          # the pair i == j, by index
    terms = [p0 * ss, two * p1 * dds, -four * p2 * q, -two * dtype(D) * p1]
    kp = (terms[0] + terms[1] + terms[2] + terms[3]) * off
    rows[i0:i0 + chunk] = kp.astype(np.float64).sum(1)
    scale_v = max(scale_v, float((sum(np.abs(t) for t in terms) * off).max()))
    a_terms = [two * p1 * ss, four * p2 * dds, -eight * p3 * q, -(eight + four * dtype(D)) * p2]
    A = (a_terms[0] + a_terms[1] + a_terms[2] + a_terms[3]) * off
    m = two * p1 * off
    cx = A[:, :, None] * d + m[:, :, None] * ds
    cs = (p0 * off)[:, :, None] * s[None, :, :] - m[:, :, None] * d
    gx[i0:i0 + chunk] = cx.astype(np.float64).sum(1)
    gs[i0:i0 + chunk] = cs.astype(np.float64).sum(1)
    absA = sum(np.abs(t) for t in a_terms) * off
    scale_gx = max(scale_gx, float((absA[:, :, None] * np.abs(d) + np.abs(m)[:, :, None] * np.abs(ds)).max()))
    scale_gs = max(scale_gs, float((np.abs(p0 * off)[:, :, None] * np.abs(s)[None] + np.abs(m)[:, :, None] * np.abs(d)).max()))
  z0, z1 = phis(np.zeros(()), sp, dtype)[:2]
  diag = float(z0) * (s.astype(np.float64) ** 2).sum(1) - 2.0 * D * float(z1)
  cg = 2.0 / (N * (N - 1.0))
  grad_s = cg * gs
  return {"sums": np.array([rows.sum(), diag.sum()]), "rows": rows / (N - 1.0), "grad_x": cg * gx, "grad_s": grad_s,
          "direction": 0.5 * (N - 1.0) * grad_s + float(z0) * s.astype(np.float64) / N,
          "scale_v": scale_v, "scale_gx": scale_gx, "scale_gs": scale_gs}


def ksd2(x, s, sp):
  """(KSD^2_U, KSD^2_V) of one set in float64"""
  r = stats(x, s, sp)
  N = len(x)
  return r["sums"][0] / (N * (N - 1.0)), (r["sums"][0] + r["sums"][1]) / (float(N) * N)
