"""float64 NumPy restatement of the permutation test of cnf_mmd_perm (include/cnf_ot_amd.h), built on mmd_ref: for
each label vector the pooled sample is split into its two subsets and mmd_ref.mmd2 is called on them -- the direct
definition, independent of the q / r / t identity the kernel uses -- with the identity itself (q, r, t of the pooled
zero-diagonal kernel matrix), the unpacker of the label words, the p-value and the inputs of the exact p-value
comparison beside it.  A helper: no tests in it.
"""
import math

import numpy as np

import mmd_ref as mr

EPS = 5e-6                                       # tests/test_gpu_mmd.py's: the value floor is 4 EPS k_max
# The inputs on which the GPU p-value is compared exactly with the restatement's; their gap condition is asserted by
# tests/test_mmd_perm_cpu.py
P_VALUE_CASES = [dict(D=2, N=96, M=80, cloud_seed=5, shift=0.25, scale=1.0, n_bw=3, n_perm=63, label_seed=1, p=3 / 64),
                 dict(D=2, N=96, M=80, cloud_seed=8, shift=0.25, scale=1.0, n_bw=3, n_perm=63, label_seed=3, p=28 / 64)]


def p_value_inputs(c):
  """(x, y, spec, label words [n, 2] as an int32 tensor) of a case of P_VALUE_CASES"""
  from cnf_ot_amd import utils
  x, y = mr.clouds(c["D"], c["N"], c["M"], seed=c["cloud_seed"], shift=c["shift"], scale=c["scale"])
  sp = mr.spec("gaussian", [float(np.float32(math.sqrt(c["D"]) * 0.5 * 2.0 ** b)) for b in range(c["n_bw"])])
  return x, y, sp, utils.permutation_labels(c["N"], c["M"], c["n_perm"], c["label_seed"])


def unpack(words):
  """Membership [n, P] (bool; True: first sample) of label words [n, P / 32]: bit b of word w is vector 32 w + b"""
  w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
  return (((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1) != 0).reshape(w.shape[0], -1)


def pack(member):
  """Label words [n, P / 32] (int32) of a membership matrix [n, P], written bit by bit"""
  member = np.asarray(member, dtype=bool)
  n, P = member.shape
  words = np.zeros((n, P // 32), dtype=np.uint32)
  for p in range(P):
    words[:, p // 32] |= member[:, p].astype(np.uint32) << np.uint32(p % 32)
  return words.view(np.int32)


def stats(x, y, sp, member):
  """The statistic under every label vector [P], by the direct definition; NaN where a side has fewer than 2 points"""
  z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
  out = np.full(member.shape[1], np.nan)
  for p in range(member.shape[1]):
    a, b = z[member[:, p]], z[~member[:, p]]
    if len(a) >= 2 and len(b) >= 2:
      out[p] = mr.mmd2(a, b, sp)
  return out


def kernel_matrix(x, y, sp):
  """The pooled sample's kernel matrix [n, n] with its diagonal zeroed"""
  z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
  k, _ = mr._kernel(z[:, None, :] - z[None, :, :], sp)
  np.fill_diagonal(k, 0.0)
  return k


def qrt(K, member):
  """(q [P], r [P], t) = (s' K s, 1' K s, 1' K 1) for the sign vectors s = +1 (first sample) / -1"""
  s = np.where(member, 1.0, -1.0)
  ks = K @ s
  return (s * ks).sum(0), ks.sum(0), K.sum()


def stats_of_qrt(q, r, t, n_first, n):
  """The statistic from q, r, t and the first sample's size [P]: the identity of DESIGN.md 5.3t"""
  n1 = np.asarray(n_first, dtype=np.float64)
  n2 = n - n1
  sxx, syy, sxy = (t + 2.0 * r + q) / 4.0, (t - 2.0 * r + q) / 4.0, (t - q) / 4.0
  with np.errstate(divide="ignore", invalid="ignore"):
    v = sxx / (n1 * (n1 - 1.0)) + syy / (n2 * (n2 - 1.0)) - 2.0 * sxy / (n1 * n2)
  return np.where((n1 >= 2) & (n2 >= 2), v, np.nan)


def p_value(observed, null):
  """(1 + #{null >= observed}) / (1 + n_perm)"""
  return (1.0 + float((np.asarray(null) >= observed).sum())) / (1.0 + len(null))
