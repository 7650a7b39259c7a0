"""float64 NumPy restatement of the wild bootstrap of cnf_stein_boot (include/cnf_ot_amd.h), built on stein_ref: for a
sign vector with A = {e = +1} and B its complement,
  q = e' H e = 2 (S_A + S_B) - t,
S_A and S_B the off-diagonal Stein kernel sums (stein_ref.stats' sums[0]) of the two subsets with their scores (a subset
with fewer than 2 points has no pair: 0) and t that of the whole set -- the direct definition, independent of the matrix
product the kernel uses -- with the product form (E * (H E)).sum itself, the packer and unpacker of the sign words, the
p-value and the inputs of the exact p-value comparison beside it.  A helper: no tests in it.
"""
import numpy as np

import stein_ref as sr

EPS = 5e-6                                       # tests/test_gpu_stein.py's: the value floor is 4 EPS scale_v
# The inputs on which the GPU p-value is compared exactly with the restatement's; their gap condition is asserted by
# tests/test_stein_boot_cpu.py.  IMQ, c = 1, beta = -1/2, D = 2: a standard normal cloud moved by `shift` along every
# axis against the score -x of N(0, I), under rademacher_signs(N, 63, sign_seed)
P_VALUE_CASES = [dict(D=2, N=96, cloud_seed=1, shift=0.15, n_boot=63, sign_seed=4, p=18 / 64),
                 dict(D=2, N=97, cloud_seed=2, shift=0.1, n_boot=63, sign_seed=2, p=25 / 64)]


def p_value_spec():
  return sr.spec("imq", [1.0])


def p_value_inputs(c):
  """(x, score, spec, sign words [N, 2] as an int32 tensor) of a case of P_VALUE_CASES"""
  from cnf_ot_amd import utils
  x = (sr.cloud(c["D"], c["N"], c["cloud_seed"]) + np.float32(c["shift"])).astype(np.float32)
  return x, -x, p_value_spec(), utils.rademacher_signs(c["N"], c["n_boot"], c["sign_seed"])


def linear_score(x, seed):
  """A score that is not proportional to x: -A x + b of a Gaussian with precision-like A = I + 0.25 G (G, b of `seed`),
  float32 like x ([N, D] or [S, N, D])"""
  D = x.shape[-1]
  rng = np.random.default_rng(seed)
  A = np.eye(D) + 0.25 * rng.standard_normal((D, D))
  b = 0.5 * rng.standard_normal(D)
  return (-(x.astype(np.float64) @ A.T) + b).astype(np.float32)


def unpack(words):
  """Signs [N, P] (bool; True: +1) of sign words [N, P / 32]: bit b of word w is vector 32 w + b"""
  w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
  return (((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1) != 0).reshape(w.shape[0], -1)


def pack(plus):
  """Sign words [N, P / 32] (int32) of a sign matrix [N, P] (True: +1), written bit by bit"""
  plus = np.asarray(plus, dtype=bool)
  n, P = plus.shape
  words = np.zeros((n, P // 32), dtype=np.uint32)
  for p in range(P):
    words[:, p // 32] |= plus[:, p].astype(np.uint32) << np.uint32(p % 32)
  return words.view(np.int32)


def _pair_sum(x, s, sp):
  return sr.stats(x, s, sp)["sums"][0] if len(x) >= 2 else 0.0


def stats(x, s, sp, plus):
  """The bootstrap of ONE set under every sign vector, by the direct definition: a dict of q [P] = e' H e, stats [P] =
  q / (N (N - 1)), t = 1' H 1, diag = sum_i k_p(x_i, x_i) and scale_v (stein_ref.stats' of the whole set)"""
  x, s = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64)
  N = len(x)
  whole = sr.stats(x, s, sp)
  t = whole["sums"][0]
  q = np.empty(plus.shape[1])
  for p in range(plus.shape[1]):
    a = plus[:, p]
    q[p] = 2.0 * (_pair_sum(x[a], s[a], sp) + _pair_sum(x[~a], s[~a], sp)) - t
  return {"q": q, "stats": q / (N * (N - 1.0)), "t": t, "diag": whole["sums"][1], "scale_v": whole["scale_v"]}


def kernel_matrix(x, s, sp, dtype=np.float64):
  """The Stein kernel matrix H [N, N] of one set with its diagonal zeroed, the pair quantities formed in dtype"""
  x, s = np.asarray(x, dtype=dtype), np.asarray(s, dtype=dtype)
  D = x.shape[1]
  d = x[:, None, :] - x[None, :, :]
  ds = s[None, :, :] - s[:, None, :]
  q = (d * d).sum(-1)
  p0, p1, p2, _ = sr.phis(q, sp, dtype)
  H = p0 * (s[:, None, :] * s[None, :, :]).sum(-1) + dtype(2.0) * p1 * (d * ds).sum(-1) - dtype(4.0) * p2 * q \
      - dtype(2.0) * dtype(D) * p1
  np.fill_diagonal(H, 0.0)
  return H


def q_product(H, plus):
  """q [P] = e' H e by the product form the kernel uses: (E * (H E)).sum over the rows, in float64"""
  e = np.where(plus, 1.0, -1.0)
  return (e * (np.asarray(H, dtype=np.float64) @ e)).sum(0)


def p_value(observed, null):
  """(1 + #{null >= observed}) / (1 + n_boot)"""
  return (1.0 + float((np.asarray(null) >= observed).sum())) / (1.0 + len(null))
