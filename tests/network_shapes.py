"""The network shapes the engine compiles kernels for, shared by the CPU and GPU
tests of every (hidden_size, num_bins) instantiation (test_network_shapes_cpu,
test_gpu_network_shapes).  Test helpers only: no tests here.

`kernel_configs()` reads CNF_KERNEL_CONFIGS from cnf_common.h itself, so an
instantiation added there is in the matrix without editing the tests.
`param_scale()` picks the N(0, s^2) parameter scale of each shape: the s at
which the conditioner outputs have the spread the default network
(hidden 16, 2 MLP layers, dim 2) has at s = 0.2, so that every shape is as
well conditioned as the default one.
"""
import os
import re
from functools import lru_cache
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_H = os.path.join(ROOT, "cnf_ot_amd", "csrc", "cnf_common.h")


@lru_cache(maxsize=None)
def kernel_configs():
  """The (hidden_size, num_bins) pairs of the full build's CNF_KERNEL_CONFIGS, in header order."""
  with open(COMMON_H) as f:
    text = f.read()
  # the full list is the #else branch of CNF_MINIMAL_CONFIGS: the last definition of the macro
  defs = re.findall(r"#define\s+CNF_KERNEL_CONFIGS\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
  assert defs, "CNF_KERNEL_CONFIGS not found in cnf_common.h"
  pairs = [(int(h), int(k)) for h, k in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", defs[-1])]
  assert pairs and len(set(pairs)) == len(pairs), pairs
  return tuple(pairs)


class Net(NamedTuple):
  H: int
  K: int
  M: int = 2      # mlp_num_layers
  L: int = 2      # flow layers

  @property
  def id(self):
    return f"h{self.H}k{self.K}m{self.M}l{self.L}"


def networks():
  """Every (H, K) pair at M = 2, L = 2; the MFMA conditioner's depth loop (16, 5) at M = 1, 3, 4; mixed shapes."""
  nets = [Net(h, k) for h, k in kernel_configs()]
  nets += [Net(16, 5, m) for m in (1, 3, 4)]
  nets += [Net(8, 5, 1), Net(64, 5, 3), Net(16, 10, 3, 3), Net(32, 5, 1, 1)]
  return nets


def flow_dims(net):
  """Dims 2 and 5 for every network; 17 (flow_dpar_kernel's 16-wave, 1024-thread block) at the extremes."""
  wide = net.M == 2 and net.L == 2 and (net.H in (8, 64) or (net.H, net.K) == (16, 10))
  return (2, 5, 17) if wide else (2, 5)


def _cond_spread(H, M, D, s, z):
  """Mean over the conditioned dimensions d = 1..D-1 of the std of the conditioner's outputs, inputs [c, x_0..x_{d-1}]
  with c ~ U(0, 1), x ~ N(0, 1); weights s * z (z: fixed standard-normal draws)."""
  out = []
  for d in range(1, D):
    zz = z[d]
    h = zz["inp"][:, :1 + d]
    for m in range(M):
      w = zz["w"][m][:h.shape[1]] * s
      h = np.maximum(h @ w + s * zz["b"][m], 0.0)
    out.append((h @ (s * zz["wo"]) + s * zz["bo"]).std())
  return float(np.mean(out))


@lru_cache(maxsize=None)
def param_scale(H, M, D):
  """N(0, s^2) scale of shape (H, M) at dim D whose conditioner outputs spread like the default network's at 0.2,
  rounded to 3 digits."""
  def draws(H, M, D):
    rng = np.random.default_rng(1234)
    z = {}
    for d in range(1, D):
      inp = np.concatenate([rng.uniform(0, 1, (2000, 1)), rng.normal(size=(2000, D))], 1)
      z[d] = dict(inp=inp, w=[rng.normal(size=(max(H, D + 1), H)) for _ in range(M)],
                  b=[rng.normal(size=H) for _ in range(M)], wo=rng.normal(size=(H, 16)), bo=rng.normal(size=16))
    return z
  target = _cond_spread(16, 2, 2, 0.2, draws(16, 2, 2))
  z = draws(H, M, D)
  lo, hi = 1e-3, 1.0
  for _ in range(40):           # the spread grows monotonically with s
    mid = np.sqrt(lo * hi)
    lo, hi = (mid, hi) if _cond_spread(H, M, D, mid, z) < target else (lo, mid)
  # ... and by sqrt(5 / D) beyond dim 5, where D - 1 conditioned splines per layer compound (the default network's own
  # tests shrink the scale the same way: 0.12 at dim 10, 0.05 at dim 24)
  return float(f"{np.sqrt(lo * hi) * min(1.0, np.sqrt(5.0 / D)):.3g}")
