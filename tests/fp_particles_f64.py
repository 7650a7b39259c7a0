"""NumPy float64 restatement of cnf_fp_particles / cnf_point_stats (include/cnf_ot_amd.h): the Euler-Maruyama ensemble of
dX = drift(X) dt + sqrt(2 sigma) dW behind flow_matching_loss_fn (applications.py:279-374), the reference the GPU tests
hold the kernels to.  Test infrastructure only.

The four drifts are written out from applications.py:309-372.  Their constants are the ones the loss kernels use
(drift_field, cnf_terms.h, the one definition on the device): `a`, 28 / 9 and 8 / 3 are float32 values, widened -- with
the float64 quotients a Lorenz path leaves the device's by 1e-8 per unit time before any rounding does.
"""
import math

import numpy as np

DRIFTS = {"ou": 0, "gradient": 1, "nongradient": 2, "lorenz": 3}
DRIFT_DIM = {"gradient": 2, "nongradient": 2, "lorenz": 3}           # ou: any
_C28_9 = float(np.float32(28.0) / np.float32(9.0))
_C8_3 = float(np.float32(8.0) / np.float32(3.0))


def drift(x, subtype, a):
  """drift(x) for x [..., D] (float64)"""
  a = float(np.float32(a))
  if subtype == "ou":                                  # :310  -a r
    return x * -a
  if subtype == "gradient":                            # :353-357, the single smiling distribution
    X, Y = x[..., 0], x[..., 1]
    q = X * X + Y * Y - 4.0
    return np.stack([(-q * X) * a, (-q * Y - (Y - 1.0) * 2.0) * a], -1)
  if subtype == "nongradient":                         # :358-363  -a r + 0.5 r @ [[0, 1], [-1, 0]]
    X, Y = x[..., 0], x[..., 1]
    return np.stack([X * -a - Y * 0.5, Y * -a + X * 0.5], -1)
  if subtype == "lorenz":                              # :364-372, _r = 9
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    return np.stack([(Y - X) * 10.0, X * 9.0 * (_C28_9 - Z) - Y, X * 9.0 * Y - Z * _C8_3], -1)
  raise ValueError(subtype)


def linear_drift_matrix(subtype, a, D):
  """A of drift(x) = A x for the two linear fields"""
  a = float(np.float32(a))
  if subtype == "ou":
    return -a * np.eye(D)
  if subtype == "nongradient":
    return np.array([[-a, -0.5], [0.5, -a]])
  raise ValueError(f"{subtype} is not linear")


def stream_stride(n_steps, D):
  """R: the stream elements a particle owns, (n_steps + 1) D rounded up to a whole number of Philox blocks"""
  return -(-(n_steps + 1) * D // 4) * 4


def particle_normals(flat, N, n_steps, D):
  """flat: the normals' stream from element first_particle * R on, at least N R of them -> z [N, n_steps + 1, D]:
  z[i, 0] draws particle i's start, z[i, k] drives its step k"""
  R = stream_stride(n_steps, D)
  return np.asarray(flat, dtype=np.float64)[:N * R].reshape(N, R)[:, :(n_steps + 1) * D].reshape(N, n_steps + 1, D)


def integrate(z, subtype, a, sigma, h, var0, snaps, x0=None):
  """pos [S, N, D] at the step indices `snaps` (ascending): x0 = sqrt(var0) z_0 (or the given x0), then
  x <- (x + h drift(x)) + sqrt(2 sigma h) z_k"""
  snaps = [int(s) for s in snaps]
  x = np.sqrt(var0) * z[:, 0] if x0 is None else np.array(x0, dtype=np.float64)
  sdn = np.sqrt(2.0 * sigma * h)
  out = []
  with np.errstate(invalid="ignore", over="ignore"):
    for k in range(snaps[-1] + 1):
      if k in snaps:
        out.append(x.copy())
      if k < snaps[-1]:
        x = (x + h * drift(x, subtype, a)) + sdn * z[:, k + 1]
  return np.stack(out)


def cell_index(x, lo, step, n):
  """The histogram cell of coordinate x: cell j is centred on lo + j step.  Returns (index, inside the grid)"""
  with np.errstate(invalid="ignore"):
    q = np.floor((x - (lo - step / 2)) / step)
    ok = (q >= 0) & (q < n)
  return np.where(ok, q, 0).astype(np.int64), ok


def stats(pos, grid=None):
  """sums [S, 2 + D + D D] (finite count, non-finite count, sum x_d, sum x_d x_e over the finite particles) and, with
  grid = dict(lo=(x, y), step=(x, y), n=(nx, ny), axes=(ax, ay)), hist [S, ny, nx] (int64; else None)"""
  pos = np.asarray(pos, dtype=np.float64)
  S, N, D = pos.shape
  sums = np.zeros((S, 2 + D + D * D))
  hist = None if grid is None else np.zeros((S, grid["n"][1], grid["n"][0]), dtype=np.int64)
  for s in range(S):
    fin = np.isfinite(pos[s]).all(1)
    x = pos[s][fin]
    sums[s, 0], sums[s, 1] = fin.sum(), N - fin.sum()
    sums[s, 2:2 + D] = x.sum(0)
    sums[s, 2 + D:] = (x[:, :, None] * x[:, None, :]).sum(0).reshape(-1)
    if grid is not None:
      jx, okx = cell_index(x[:, grid["axes"][0]], grid["lo"][0], grid["step"][0], grid["n"][0])
      jy, oky = cell_index(x[:, grid["axes"][1]], grid["lo"][1], grid["step"][1], grid["n"][1])
      ok = okx & oky
      np.add.at(hist[s], (jy[ok], jx[ok]), 1)
  return sums, hist


def abs_sums(pos):
  """sum |term| per entry of `stats`' sums: the scale of their rounding error"""
  return stats(np.abs(np.where(np.isfinite(pos).all(2, keepdims=True), pos, np.nan)))[0]


def moments(sums, D):
  """(count, mean [S, D], cov [S, D, D]) from raw sums: cov = sum x x^T / count - mean mean^T"""
  n = sums[:, 0]
  mean = sums[:, 2:2 + D] / n[:, None]
  cov = sums[:, 2 + D:].reshape(-1, D, D) / n[:, None, None] - mean[:, :, None] * mean[:, None, :]
  return n, mean, cov


def em_moments(A, mean0, cov0, sigma, h, k):
  """Mean and covariance after k Euler-Maruyama steps of a linear drift A x: exact for the scheme (the continuous
  closed form, applications.ou_variance, is not): m <- (I + h A) m, C <- (I + h A) C (I + h A)^T + 2 sigma h I"""
  M = np.eye(A.shape[0]) + h * A
  m, C = np.array(mean0, dtype=np.float64), np.array(cov0, dtype=np.float64)
  for _ in range(k):
    m, C = M @ m, M @ C @ M.T + 2.0 * sigma * h * np.eye(A.shape[0])
  return m, C


def em_ou_variance(v, a, sigma, h, k):
  """v <- (1 - a h)^2 v + 2 sigma h, k times"""
  for _ in range(k):
    v = (1.0 - a * h) ** 2 * v + 2.0 * sigma * h
  return v


# The Ornstein-Uhlenbeck statistics check that the CPU test runs on the restatement and the GPU test on the kernel
OU = dict(N=65536, D=2, a=1.0, sigma=0.5, var0=1.0, h=0.01, n_steps=100, snaps=(0, 50, 100))
OU_SEED = 1


def ou_check(count, mean, cov, what, units=5.0):
  """The three Ornstein-Uhlenbeck bounds on per-snapshot count [S], mean [S, D], cov [S, D, D]; prints the figures in
  units of the standard errors."""
  N, D = OU["N"], OU["D"]
  worst = 0.0
  for s, k in enumerate(OU["snaps"]):
    v = em_ou_variance(OU["var0"], OU["a"], OU["sigma"], OU["h"], k)
    assert count[s] == N
    e_var = np.abs(np.diag(cov[s]) - v).max() / (v * math.sqrt(2.0 / (N - 1)))
    e_mean = np.abs(mean[s]).max() / math.sqrt(v / N)
    e_off = abs(cov[s][0, 1]) / (v / math.sqrt(N))
    print(f"[{what} step {k}] v = {v:.6f}: variance {e_var:.2f}, mean {e_mean:.2f}, off-diagonal {e_off:.2f} standard errors")
    for name, e in (("variance", e_var), ("mean", e_mean), ("off-diagonal", e_off)):
      assert e <= units, (what, k, name, e)
    worst = max(worst, e_var, e_mean, e_off)
  return worst
