"""A float64 NumPy restatement of cnf_knn and of the estimators built on it (include/cnf_ot_amd.h), written from the
formulas and independent of cnf_ot_amd.two_sample: brute force over all pairs, neighbours ordered by a stable sort on
(d2, index).  The inputs are float32 arrays; the restatement reads the same float32 values as float64.

  neighbours(x, y, k)  (d2 [N, k], idx [N, k]): y None = the other points of x (the diagonal left out by index)
  sums_of(d2)          [k, 2]: per rank, sum of 0.5 log d2 over the rows with d2 > 0, and the rows with d2 == 0
  estimates(...)       entropy, cross entropy and KL per rank from such sums
  exact_grid / gaussian  clouds: coordinates that are multiples of 1/8 in [-4, 4] (every d2 is then exact in float32 --
                         at most 14 * 64 * 64 units of 1/64 -- and ties and duplicates are plentiful), and Gaussian ones
  GAUSSIAN_CASES, gaussian_case, gaussian_reference, index_rule  what the CPU and the GPU test share
"""
import functools
import math

import numpy as np

EULER_GAMMA = 0.57721566490153286061


def exact_grid(D, N, seed, S=None):
  """float32 [N, D] ([S, N, D]): multiples of 1/8 in [-4, 4]"""
  rng = np.random.default_rng(seed)
  return (rng.integers(-32, 33, size=((N, D) if S is None else (S, N, D))) / 8.0).astype(np.float32)


def gaussian(D, N, seed, mean=0.0, scale=1.0, S=None):
  """float32 [N, D] ([S, N, D]): mean + scale * N(0, I), rounded to float32"""
  rng = np.random.default_rng(seed)
  return (mean + scale * rng.standard_normal((N, D) if S is None else (S, N, D))).astype(np.float32)


def pair_d2(x, y):
  """[N, M] float64: squared distances, one dimension at a time (no [N, M, D] array)"""
  x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
  d2 = np.zeros((len(x), len(y)))
  for d in range(x.shape[1]):
    diff = x[:, d, None] - y[None, :, d]
    d2 += diff * diff
  return d2


def neighbours(x, y, k):
  """(d2 [N, k] float64, idx [N, k] int64), ascending by (d2, index); y None: among the other points of x"""
  d2 = pair_d2(x, x if y is None else y)
  if y is None:
    np.fill_diagonal(d2, np.inf)
  assert d2.shape[1] - (y is None) >= k
  kth = np.partition(d2, k - 1, axis=1)[:, k - 1]
  idx = np.empty((len(d2), k), dtype=np.int64)
  for i in range(len(d2)):
    c = np.flatnonzero(d2[i] <= kth[i])                  # ascending index: the stable sort keeps it among equal d2
    idx[i] = c[np.argsort(d2[i, c], kind="stable")][:k]
  return np.take_along_axis(d2, idx, axis=1), idx


def dist_f32(d2):
  """The distances as cnf_knn writes them: (float)sqrt((double)d2), for a d2 that float32 holds exactly"""
  return np.sqrt(d2).astype(np.float32)


def sums_of(d2):
  """[k, 2] float64: (sum over the rows with d2 > 0 of 0.5 log d2, the rows with d2 == 0), per rank"""
  pos = d2 > 0.0
  logs = np.where(pos, 0.5 * np.log(np.where(pos, d2, 1.0)), 0.0)
  return np.stack([np.array([math.fsum(logs[:, j]) for j in range(d2.shape[1])]), (d2 == 0.0).sum(0).astype(np.float64)], 1)


def digamma_int(n):
  """psi(n) for an integer n >= 1: -gamma + sum_{m < n} 1 / m"""
  return -EULER_GAMMA + math.fsum(1.0 / m for m in range(1, int(n)))


def log_unit_ball(D):
  return 0.5 * D * math.log(math.pi) - math.lgamma(0.5 * D + 1.0)


def estimates(sums, N, M, D):
  """sums [2, k, 2] (self, cross) -> dict of [k] arrays: entropy, cross_entropy, kl (None, None without M)"""
  sums = np.asarray(sums, dtype=np.float64)
  k = sums.shape[1]
  psi_j = np.array([digamma_int(j) for j in range(1, k + 1)])
  mean = sums[:, :, 0] / (N - sums[:, :, 1])
  ent = digamma_int(N) - psi_j + log_unit_ball(D) + D * mean[0]
  if not M:
    return {"entropy": ent, "cross_entropy": None, "kl": None}
  cross = math.log(M) - psi_j + log_unit_ball(D) + D * mean[1]
  return {"entropy": ent, "cross_entropy": cross, "kl": cross - ent}


def estimates_of_clouds(x, y, k):
  """The estimators of one set, straight from the clouds"""
  s = np.stack([sums_of(neighbours(x, None, k)[0]), sums_of(neighbours(x, y, k)[0])])
  return estimates(s, len(x), len(y), x.shape[1])


# ---- what the GPU test's Gaussian cases and the CPU test of the index rule share ---------------------------------------

GAUSSIAN_CASES = [(2, 700, 1100), (3, 257, 130), (10, 300, 257), (14, 129, 64)]      # (D, N, M); k = 4 and 16
GAUSSIAN_KS = (4, 16)


def distance_bound(D):
  """Relative error of a float32 distance against the float64 one: one rounding per difference, three per
  square-and-add, and the square root halves it -- (D + 4) 2^-24 with room for the root's own rounding"""
  return (D + 4) * 2.0 ** -24


def gaussian_case(D, N, M):
  index = GAUSSIAN_CASES.index((D, N, M))
  return gaussian(D, N, 3000 + index), gaussian(D, M, 4000 + index, mean=0.5, scale=1.25)


@functools.lru_cache(maxsize=None)
def gaussian_reference(D, N, M, k):
  """((d2, idx) of the self block, (d2, idx) of the cross block), each with k + 1 ranks where the cloud has them (the
  extra rank is what index_rule compares rank k with)"""
  x, y = gaussian_case(D, N, M)
  return neighbours(x, None, min(k + 1, N - 1)), neighbours(x, y, min(k + 1, M))


def index_rule(d2, k, bound):
  """[N, k] bool: the (row, rank) entries whose index a float32 scan must reproduce -- the distance's gap to both
  neighbouring ranks exceeds twice `bound` (relative).  d2: [N, k] or [N, k + 1]"""
  d = np.sqrt(d2)
  below = np.concatenate([np.full((len(d), 1), -np.inf), d[:, :-1]], 1)[:, :k]
  above = np.concatenate([d[:, 1:], np.full((len(d), 1), np.inf)], 1)[:, :k]
  dj = d[:, :k]
  return (dj - below > 2.0 * bound * dj) & (above - dj > 2.0 * bound * above)
