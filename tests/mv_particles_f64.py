"""NumPy float64 restatement of cnf_mv_particles (include/cnf_ot_amd.h): R independent replicas of N particles,
  x_i <- (x_i + h (drift(x_i) - kappa G_i)) + sqrt(2 sigma h) z,   G_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j),
the interacting particle system behind d rho / dt = -div(rho (drift - kappa grad (W * rho))) + sigma lap rho.  The drift,
the stream layout and the statistics are fp_particles_f64's, the pair kernel interaction_ref's; the force is float64 on
the float32 ROUNDING of the positions, which is what the device's pair pass reads.  A helper: no tests in it.
"""
import numpy as np

import fp_particles_f64 as fp
import interaction_ref as ir

EPS32 = 5e-6          # test_gpu_interaction.py's EPS: the float32 pair sums' floor, in units of k_max (value) or tau (force)


def rounded(x):
  """The float32 rounding of the positions, widened: what the pair pass sees"""
  with np.errstate(over="ignore", invalid="ignore"):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def force_f64(x, sp):
  """(G [N, D], sum_i sum_{j != i} W) of one replica x [N, D]: float64 on the rounded positions"""
  _, G, total, _ = ir.rows(rounded(x), sp)
  return G, total


def force_f32(x, sp):
  """The same composed in NumPy float32 throughout -- differences, distances, the kernel, the products and their sums
  over the columns -- and widened at the end: the composition a float32 array program gives"""
  x32 = np.asarray(x, dtype=np.float64).astype(np.float32)
  N = len(x32)
  f = np.float32
  G, total = np.empty(x32.shape, dtype=np.float32), 0.0
  for i0 in range(0, N, ir.CHUNK):
    diff = x32[i0:i0 + ir.CHUNK, None, :] - x32[None, :, :]
    d2 = (diff * diff).sum(-1, dtype=np.float32)
    if sp["kind"] == "quadratic":
      W, w = f(0.5 * sp["amp"][0]) * d2, np.full_like(d2, f(sp["amp"][0]))
    else:
      W, w = np.zeros_like(d2), np.zeros_like(d2)
      if sp["kind"] == "gaussian":
        for a, b in zip(sp["amp"], sp["bw"]):
          e = f(a) * np.exp(-d2 / f(2.0 * b * b))
          W += e
          w -= e / f(b * b)
      else:
        r = np.sqrt(d2)
        inv = np.where(r > 0, f(1.0) / np.where(r > 0, r, f(1.0)), f(0.0))
        for a, b in zip(sp["amp"], sp["bw"]):
          e = f(a) * np.exp(-r / f(b))
          W += e
          w -= e / f(b) * inv
    rr = np.arange(len(W))
    W[rr, i0 + rr] = 0.0
    w[rr, i0 + rr] = 0.0
    assert W.dtype == w.dtype == diff.dtype == np.float32
    G[i0:i0 + ir.CHUNK] = (diff * w[:, :, None]).sum(1, dtype=np.float32) / f(N - 1)
    total += float(W.sum(dtype=np.float32))
  return G.astype(np.float64), total


def replica_normals(flat, R, N, n_steps, D):
  """flat: the stream from element first_particle * stride on -> z [R, N, n_steps + 1, D] (global particle r N + i)"""
  return fp.particle_normals(flat, R * N, n_steps, D).reshape(R, N, n_steps + 1, D)


def integrate(z, subtype, a, sigma, h, var0, kappa, sp, snaps, x0=None, force=force_f64):
  """(pos [S, R, N, D], wsum [S, R]) at the step indices `snaps` (ascending) for normals z [R, N, n_steps + 1, D]:
  x0 = sqrt(var0) z_0 (or the given x0 [R, N, D]); wsum = sum_i sum_{j != i} W at the snapshot, from `force`"""
  snaps = [int(s) for s in snaps]
  z = np.asarray(z, dtype=np.float64)
  x = np.sqrt(var0) * z[:, :, 0] if x0 is None else np.array(x0, dtype=np.float64)
  sdn = np.sqrt(2.0 * sigma * h)
  pos, wsum = [], []
  for k in range(snaps[-1] + 1):
    fw = [force(x[r], sp) for r in range(len(x))]
    if k in snaps:
      pos.append(x.copy())
      wsum.append([t for _, t in fw])
    if k < snaps[-1]:
      G = np.stack([g for g, _ in fw])
      x = (x + h * (fp.drift(x, subtype, a) - kappa * G)) + sdn * z[:, :, k + 1]
  return np.stack(pos), np.asarray(wsum)


def energy(wsum, N):
  return np.asarray(wsum) / (2.0 * N * (N - 1.0))


def em_deviation_variance(var0, a, kappa_amp, sigma, h, N, k):
  """The EXACT expectation of the per-coordinate variance of the deviations y_i = x_i - mean_j x_j after k steps of
  drift ou with the quadratic kernel: y' = c y + sdn (z - mean z), c = 1 - h (a + kappa amp N / (N - 1)), so
  v <- c^2 v + 2 sigma h (1 - 1 / N) from v_0 = var0 (1 - 1 / N)"""
  c = 1.0 - h * (a + kappa_amp * N / (N - 1.0))
  v = var0 * (1.0 - 1.0 / N)
  for _ in range(k):
    v = c * c * v + 2.0 * sigma * h * (1.0 - 1.0 / N)
  return v
