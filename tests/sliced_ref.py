"""float64 NumPy restatement of cnf_sliced_w2 (include/cnf_ot_amd.h): the sliced Wasserstein distance between two point
clouds with uniform weights for given directions, its per-projection values and the envelope gradient in x.  A helper:
no tests in it.

  keys    float32, in the header's order: k = x[:, 0] theta[0], then k = fmaf(x[:, d], theta[d], k) in ascending d -- a
          fused multiply-add is the float64 product plus sum (the product of two float32 is exact in float64), rounded
          once to float32 -- and a key that is not finite is NaN
  order   by (the key's order-preserving unsigned image, the sample's index): ties by index, -0 below +0, a NaN by its
          bits -- one integer sort, as the kernel's
  value   w = 1/2 sum over the merged breakpoints of the two quantile functions: the segments between consecutive cuts
          of {i M} and {j N} in [0, N M], each of length len / (N M) on ranks (cut // M, cut // N).  This is the header's
          sum_i sum_j o_ij (k_(i) - l_(j))^2 / 2 written without the pair (i, j) loop.
  a       sum_j o_ij (k_i - l_j) at the rank a sample took;  grad = (1 / P) sum_p a[p, :, None] theta[p]
"""
import numpy as np


def keys(pts, theta):
  """[P, n] float32 keys of pts [n, D] under theta [P, D], both taken as float32"""
  pts = np.asarray(pts, dtype=np.float32).astype(np.float64)
  theta = np.asarray(theta, dtype=np.float32).astype(np.float64)
  with np.errstate(invalid="ignore", over="ignore"):
    k = (pts[None, :, 0] * theta[:, None, 0]).astype(np.float32)
    for d in range(1, pts.shape[1]):
      k = (pts[None, :, d] * theta[:, None, d] + k.astype(np.float64)).astype(np.float32)
  return np.where(np.isfinite(k), k, np.float32(np.nan)).astype(np.float32)


def order(k):
  """The permutation that sorts the float32 keys k [n] by (image, index): perm[rank] = sample"""
  b = np.ascontiguousarray(k, dtype=np.float32).view(np.uint32)
  image = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint64)
  return np.argsort((image << np.uint64(32)) | np.arange(len(k), dtype=np.uint64), kind="stable")


def segments(N, M):
  """The merged breakpoints: (rank of x [n_seg], rank of y [n_seg], o [n_seg] = length / (N M)), all from integers"""
  cuts = np.union1d(np.arange(N, dtype=np.int64) * M, np.arange(M, dtype=np.int64) * N)
  length = np.diff(np.append(cuts, np.int64(N) * M))
  return cuts // M, cuts // N, length.astype(np.float64) / float(N * M)


def overlap(i, j, N, M):
  """o_ij as the header writes it"""
  return max(0, min((i + 1) * M, (j + 1) * N) - max(i * M, j * N)) / float(N * M)


def one(kx, ky):
  """One projection from its float32 keys: (w, a [N] by SAMPLE, perm_x, perm_y)"""
  N, M = len(kx), len(ky)
  px, py = order(kx), order(ky)
  sx, sy = kx[px].astype(np.float64), ky[py].astype(np.float64)
  ix, iy, o = segments(N, M)
  with np.errstate(invalid="ignore"):
    diff = sx[ix] - sy[iy]
    w = 0.5 * float(np.sum(o * diff * diff))
    a_rank = np.zeros(N)
    np.add.at(a_rank, ix, o * diff)
  a = np.empty(N)
  a[px] = a_rank
  return w, a, px, py


def run(x, y, theta):
  """One set.  A dict: w [P], sw, max_sliced, sums [P + 2] as cnf_sliced_w2 writes them, a [P, N], grad [N, D] (float64),
  kx [P, N] and ky [P, M] (the float32 keys), perm_x [P, N], perm_y [P, M]"""
  theta = np.asarray(theta, dtype=np.float32)
  kx, ky = keys(x, theta), keys(y, theta)
  P, N = kx.shape
  w, a, px, py = np.empty(P), np.empty((P, N)), [], []
  for p in range(P):
    w[p], a[p], qx, qy = one(kx[p], ky[p])
    px.append(qx)
    py.append(qy)
  sw = float(np.sum(w)) / P
  mx = float(np.nan) if np.isnan(w).any() else float(w.max())
  grad = (a[:, :, None] * theta.astype(np.float64)[:, None, :]).sum(0) / P
  if np.isnan(sw):
    grad = np.full_like(grad, np.nan)
  return {"w": w, "sw": sw, "max_sliced": mx, "sums": np.concatenate([w, [sw, mx]]), "a": a, "grad": grad, "kx": kx, "ky": ky,
          "perm_x": np.stack(px), "perm_y": np.stack(py)}


def value64(x, y, theta):
  """SW of float64 clouds with float64 keys (no float32 rounding anywhere): for central differences"""
  x, y, theta = (np.asarray(v, dtype=np.float64) for v in (x, y, theta))
  ix, iy, o = segments(len(x), len(y))
  total = 0.0
  for th in theta:
    sx, sy = np.sort(x @ th), np.sort(y @ th)
    total += 0.5 * float(np.sum(o * (sx[ix] - sy[iy]) ** 2))
  return total / len(theta)


def clouds_exact(D, N, M, seed, S=None):
  """Clouds on a grid: coordinates are multiples of 2^-7 in [-8, 8).  With directions_exact every product is a multiple
  of 2^-16 below 8 in size and every partial sum of at most 14 of them is below 2^7: 23 bits and a sign, so the float32
  key is exact under any operation order and every sort of it finds the same permutation."""
  rng = np.random.default_rng(seed)
  lead = () if S is None else (S,)
  x = rng.integers(-1024, 1024, lead + (N, D)).astype(np.float32) / np.float32(128.0)
  y = rng.integers(-1024, 1024, lead + (M, D)).astype(np.float32) / np.float32(128.0)
  return x, y


def directions_exact(D, P, seed):
  """[P, D] float32 with components that are multiples of 2^-9 in [-1, 1] (not unit vectors: the kernel does not ask)"""
  rng = np.random.default_rng(seed + 977)
  return rng.integers(-512, 513, (P, D)).astype(np.float32) / np.float32(512.0)


def clouds(D, N, M, seed, shift=0.3, scale=1.2, S=None):
  """Ordinary inputs: x ~ N(0, I), y ~ N(shift (1, ..., 1), scale^2 I), rounded to float32 ([S, ., D] with S)"""
  rng = np.random.default_rng(seed)
  lead = () if S is None else (S,)
  x = rng.standard_normal(lead + (N, D)).astype(np.float32)
  y = (shift + scale * rng.standard_normal(lead + (M, D))).astype(np.float32)
  return x, y


# The "ordinary inputs" cases of the GPU tests: (D, N, M, P) and the seed of `clouds` / of utils.sliced_directions
ORDINARY = {2: (2048, 1500, 8, 3102), 10: (2048, 1500, 8, 3110)}


def ranks(perm):
  """rank[..., sample] of a permutation perm[..., rank]"""
  perm = np.asarray(perm)
  r = np.empty_like(perm)
  np.put_along_axis(r, perm, np.broadcast_to(np.arange(perm.shape[-1]), perm.shape), axis=-1)
  return r


def rows_that_agree(perm_ref, perm_other):
  """[n] bool: the samples that took the same rank under every projection in both [P, n] permutations"""
  return (ranks(perm_ref) == ranks(perm_other)).all(0)
