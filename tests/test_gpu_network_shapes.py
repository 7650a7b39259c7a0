"""Every compiled network shape against the float64 oracle.

The engine instantiates its kernels for each (hidden_size, num_bins) pair of CNF_KERNEL_CONFIGS (read from
cnf_common.h by tests/network_shapes.py) and takes mlp_num_layers 1..16 at run time.  The rest of the suite runs the
default network (hidden 16, 5 bins, 2 MLP layers) almost everywhere; this module runs every pair, the MFMA
conditioner's depth loop at M = 1, 3, 4 and a few mixed shapes through:
  - every flow kernel variant, both directions, forced with the engine knobs and pinned with last_path(): the
    one- and two-sample-per-lane kernels, ocml math, the MFMA conditioner, the wave-per-dimension kernel, the precise
    and the plain fp32 data -> base positions, the float64 kernels and the periodized kernel;
  - ragged batches, B = 1, B < 64, and launches past the grid cap (num_cus * 8 blocks: the grid-stride loops);
  - the fused loss kernel's terms (oracle/losses.py), seeded == tensor terms;
  - the entry points that must refuse these shapes (tables, gradients).

Parameters: N(0, s^2) with s = network_shapes.param_scale(H, M, D), the scale at which the conditioner outputs spread
like the default network's at 0.2 (printed with each case).  Bars: those of the default network in test_gpu_parity /
test_gpu_losses / test_gpu_evaluate, at the same dimension and flow depth (the log-density bars of the default
network grow with the number of splines summed: x2 at dim 10, x5 beyond, x L/2 for L > 2 flow layers).
"""
import functools

import numpy as np
import pytest
import torch

from network_shapes import Net, flow_dims, kernel_configs, networks, param_scale
from test_gpu_evaluate import TOL as TOL_L2, _mix64, _want
from test_gpu_parity import (TOL_LD, TOL_LP_DATA_MAX, TOL_LP_FP32_MAX, TOL_LP_FP32_P999, TOL_LP_SAMPLE, TOL_Y, _err,
                             _t)

pytestmark = pytest.mark.gpu

# float64 kernels: |d| / max(1, |ref|).  The oracle gets min_bin_size and min_knot_slope rounded to float32, as the
# C ABI carries them (_cfgs): with the exact 1e-4 the oracle itself moves by up to 1.2e-10 (h32k8m2l2 dim 2 log-det).
TOL_F64 = 1e-12
# data -> base with plain fp32 positions: x carries the ~2e-6 |x| position error of fp32 softmax-normalised knots
# (test_gpu_parity's header), |x| <= 5 on these inputs: 2.5x TOL_Y.  Its log-det is held to log_prob's fp32 bar.
TOL_X_FP32 = 5e-5
DEFAULT = Net(16, 5)
B_MAIN = 4096 + 37         # ragged for one (256) and two (512) samples per lane
B_SMALL = (37, 1)
C_SMALL = 0.37

_WORST = {}                # (network id, dim, family) -> worst error / bar

# Loosened bars, one per measured case: (network, dim, family, quantity) -> (max bar, p99.9 bar); None keeps the bar of
# the default network.  Each case missed that bar, and the oracle's own float32 port, on the same inputs, misses it
# alike: the comment gives the kernel's median, p99, max (p99.9 where that bar moved) | the port's median, p99, max.
# Each bar is 1.2x the measured maximum, at most 2x the port's maximum.  _Case.check also holds such a case to 2x the
# port's median and p99.  All are at dims 2 and 5 (at dim 5 four conditioned splines per layer add up; the default
# network is never tested there); the default network and every launch past the grid cap keep their bars.
LOOSENED = {
  ("h16k4m2l2", 5, "base->data mlp1", "logdet"):
    (1.3e-05, None),  # 3.84e-07 2.82e-06 1.01e-05 | 4.99e-07 3.22e-06 6.77e-06
  ("h16k4m2l2", 5, "base->data mlp2", "logdet"):
    (1.3e-05, None),  # 3.84e-07 2.82e-06 1.01e-05 | 4.99e-07 3.22e-06 6.77e-06
  ("h16k10m2l2", 5, "base->data ocml1", "logdet"):
    (1.3e-05, None),  # 8.32e-07 5.69e-06 1.07e-05 | 1.23e-06 7.10e-06 1.16e-05
  ("h32k5m2l2", 5, "base->data mlp1", "logdet"):
    (1.7e-05, None),  # 4.31e-07 4.23e-06 1.63e-05 | 9.26e-07 4.98e-06 8.71e-06
  ("h32k5m2l2", 5, "base->data mlp1", "log_prob"):
    (1.8e-05, None),  # 0.00e+00 3.27e-06 1.48e-05 | 9.53e-07 4.95e-06 9.61e-06
  ("h32k5m2l2", 5, "base->data mlp2", "logdet"):
    (1.7e-05, None),  # 4.31e-07 4.23e-06 1.63e-05 | 9.26e-07 4.98e-06 8.71e-06
  ("h32k5m2l2", 5, "base->data mlp2", "log_prob"):
    (1.8e-05, None),  # 0.00e+00 3.27e-06 1.48e-05 | 9.53e-07 4.95e-06 9.61e-06
  ("h32k5m2l2", 5, "base->data ocml1", "logdet"):
    (1.7e-05, None),  # 4.27e-07 4.53e-06 1.60e-05 | 9.26e-07 4.98e-06 8.71e-06
  ("h32k5m2l2", 5, "base->data ocml1", "log_prob"):
    (1.8e-05, None),  # 0.00e+00 3.47e-06 1.43e-05 | 9.53e-07 4.95e-06 9.61e-06
  ("h32k5m2l2", 5, "base->data dpar1", "logdet"):
    (1.7e-05, None),  # 4.25e-07 4.27e-06 1.65e-05 | 9.26e-07 4.98e-06 8.71e-06
  ("h32k5m2l2", 5, "base->data dpar1", "log_prob"):
    (1.9e-05, None),  # 0.00e+00 3.28e-06 1.53e-05 | 9.53e-07 4.95e-06 9.61e-06
  ("h32k5m2l2", 5, "base->data dpar2", "logdet"):
    (1.7e-05, None),  # 4.25e-07 4.27e-06 1.65e-05 | 9.26e-07 4.98e-06 8.71e-06
  ("h32k5m2l2", 5, "base->data dpar2", "log_prob"):
    (1.9e-05, None),  # 0.00e+00 3.28e-06 1.53e-05 | 9.53e-07 4.95e-06 9.61e-06
  ("h32k5m2l2", 5, "data->base mlp1", "x"):
    (3e-05, None),  # 2.99e-07 4.06e-06 2.44e-05 | 1.96e-06 1.38e-05 3.30e-05
  ("h32k5m2l2", 5, "data->base mlp1", "log_prob"):
    (4.2e-05, None),  # 0.00e+00 9.40e-06 3.50e-05 | 4.20e-06 3.37e-05 9.35e-05
  ("h32k5m2l2", 5, "data->base mlp1 fp32", "log_prob"):
    (None, 3.6e-05),  # 1.34e-06 1.86e-05 4.41e-05 (p99.9 2.99e-05) | 4.20e-06 3.37e-05 9.35e-05
  ("h32k5m2l2", 5, "data->base mlp2", "x"):
    (3e-05, None),  # 2.99e-07 4.06e-06 2.44e-05 | 1.96e-06 1.38e-05 3.30e-05
  ("h32k5m2l2", 5, "data->base mlp2", "log_prob"):
    (4.2e-05, None),  # 0.00e+00 9.40e-06 3.50e-05 | 4.20e-06 3.37e-05 9.35e-05
  ("h32k5m2l2", 5, "data->base mlp2 fp32", "log_prob"):
    (None, 3.6e-05),  # 1.34e-06 1.86e-05 4.41e-05 (p99.9 2.99e-05) | 4.20e-06 3.37e-05 9.35e-05
  ("h32k5m2l2", 5, "data->base ocml1", "x"):
    (2.8e-05, None),  # 2.97e-07 4.02e-06 2.33e-05 | 1.96e-06 1.38e-05 3.30e-05
  ("h32k5m2l2", 5, "data->base ocml1", "log_prob"):
    (3.9e-05, None),  # 0.00e+00 9.40e-06 3.22e-05 | 4.20e-06 3.37e-05 9.35e-05
  ("h32k5m2l2", 5, "data->base ocml1 fp32", "log_prob"):
    (6.6e-05, 4.6e-05),  # 1.24e-06 1.81e-05 5.44e-05 (p99.9 3.76e-05) | 4.20e-06 3.37e-05 9.35e-05
  ("h32k8m2l2", 2, "base->data mlp1", "logdet"):
    (2.2e-05, None),  # 3.14e-07 3.54e-06 1.83e-05 | 4.67e-07 3.36e-06 1.81e-05
  ("h32k8m2l2", 2, "base->data mlp1", "log_prob"):
    (2.2e-05, None),  # 0.00e+00 3.15e-06 1.76e-05 | 4.78e-07 3.40e-06 1.82e-05
  ("h32k8m2l2", 2, "base->data mlp2", "logdet"):
    (2.2e-05, None),  # 3.14e-07 3.54e-06 1.83e-05 | 4.67e-07 3.36e-06 1.81e-05
  ("h32k8m2l2", 2, "base->data mlp2", "log_prob"):
    (2.2e-05, None),  # 0.00e+00 3.15e-06 1.76e-05 | 4.78e-07 3.40e-06 1.82e-05
  ("h32k8m2l2", 2, "base->data ocml1", "logdet"):
    (2e-05, None),  # 3.12e-07 3.43e-06 1.66e-05 | 4.67e-07 3.36e-06 1.81e-05
  ("h32k8m2l2", 2, "base->data ocml1", "log_prob"):
    (1.9e-05, None),  # 0.00e+00 2.95e-06 1.56e-05 | 4.78e-07 3.40e-06 1.82e-05
  ("h32k8m2l2", 5, "data->base mlp1 fp32", "log_prob"):
    (6.6e-05, 4.1e-05),  # 2.19e-06 1.98e-05 5.50e-05 (p99.9 3.36e-05) | 3.35e-06 2.19e-05 5.11e-05
  ("h32k8m2l2", 5, "data->base mlp2 fp32", "log_prob"):
    (6.6e-05, 4.1e-05),  # 2.19e-06 1.98e-05 5.50e-05 (p99.9 3.36e-05) | 3.35e-06 2.19e-05 5.11e-05
  ("h32k8m2l2", 5, "data->base ocml1 fp32", "log_prob"):
    (8.2e-05, 3.8e-05),  # 2.17e-06 1.92e-05 6.80e-05 (p99.9 3.16e-05) | 3.35e-06 2.19e-05 5.11e-05
  ("h16k5m1l2", 5, "base->data mlp1", "logdet"):
    (3.3e-05, None),  # 4.59e-07 2.61e-06 2.76e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data mlp1", "log_prob"):
    (3.1e-05, None),  # 0.00e+00 1.07e-06 2.55e-05 | 7.13e-07 3.23e-06 1.73e-05
  ("h16k5m1l2", 5, "base->data mlp2", "logdet"):
    (3.3e-05, None),  # 4.59e-07 2.61e-06 2.76e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data mlp2", "log_prob"):
    (3.1e-05, None),  # 0.00e+00 1.07e-06 2.55e-05 | 7.13e-07 3.23e-06 1.73e-05
  ("h16k5m1l2", 5, "base->data ocml1", "logdet"):
    (1.4e-05, None),  # 4.24e-07 2.74e-06 1.09e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data mfma1", "logdet"):
    (3.3e-05, None),  # 4.59e-07 2.80e-06 3.29e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data mfma1", "log_prob"):
    (3.4e-05, None),  # 0.00e+00 1.16e-06 3.12e-05 | 7.13e-07 3.23e-06 1.73e-05
  ("h16k5m1l2", 5, "base->data mfma2", "logdet"):
    (3.3e-05, None),  # 4.59e-07 2.80e-06 3.29e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data mfma2", "log_prob"):
    (3.4e-05, None),  # 0.00e+00 1.16e-06 3.12e-05 | 7.13e-07 3.23e-06 1.73e-05
  ("h16k5m1l2", 5, "base->data dpar1", "logdet"):
    (3.3e-05, None),  # 4.62e-07 2.60e-06 2.76e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data dpar1", "log_prob"):
    (3.1e-05, None),  # 0.00e+00 1.06e-06 2.55e-05 | 7.13e-07 3.23e-06 1.73e-05
  ("h16k5m1l2", 5, "base->data dpar2", "logdet"):
    (3.3e-05, None),  # 4.62e-07 2.60e-06 2.76e-05 | 6.69e-07 3.10e-06 1.68e-05
  ("h16k5m1l2", 5, "base->data dpar2", "log_prob"):
    (3.1e-05, None),  # 0.00e+00 1.06e-06 2.55e-05 | 7.13e-07 3.23e-06 1.73e-05
  ("h8k5m1l2", 5, "data->base mlp1 fp32", "log_prob"):
    (None, 3.1e-05),  # 7.45e-07 1.35e-05 4.22e-05 (p99.9 2.51e-05) | 2.70e-06 1.73e-05 3.49e-05
  ("h8k5m1l2", 5, "data->base mlp2 fp32", "log_prob"):
    (None, 3.1e-05),  # 7.45e-07 1.35e-05 4.22e-05 (p99.9 2.51e-05) | 2.70e-06 1.73e-05 3.49e-05
  ("h8k5m1l2", 5, "data->base ocml1 fp32", "log_prob"):
    (None, 3e-05),  # 6.01e-07 1.37e-05 4.68e-05 (p99.9 2.44e-05) | 2.70e-06 1.73e-05 3.49e-05
  ("h64k5m3l2", 5, "data->base mlp1 fp32", "log_prob"):
    (None, 2.7e-05),  # 1.66e-06 1.39e-05 3.39e-05 (p99.9 2.24e-05) | 2.93e-06 1.72e-05 3.71e-05
  ("h64k5m3l2", 5, "data->base mlp2 fp32", "log_prob"):
    (None, 2.7e-05),  # 1.66e-06 1.39e-05 3.39e-05 (p99.9 2.24e-05) | 2.93e-06 1.72e-05 3.71e-05
  ("h64k5m3l2", 5, "data->base ocml1 fp32", "log_prob"):
    (None, 3.1e-05),  # 1.53e-06 1.36e-05 3.46e-05 (p99.9 2.53e-05) | 2.93e-06 1.72e-05 3.71e-05
}


@pytest.fixture(scope="module", autouse=True)
def _full_build():
  """A --minimal build has only the default network's kernels: every case here would be refused.  Fail, loudly."""
  from cnf_ot_amd import _capi, build
  lib = _capi.lib()
  missing = []
  for h, k in kernel_configs():
    cfg = _capi.CnfConfig()
    lib.cnf_config_default(cfg, 2)
    cfg.hidden_size, cfg.num_bins = h, k
    if lib.cnf_config_supported(cfg) != 1:
      missing.append((h, k))
  if missing:
    pytest.fail(f"the loaded library has no kernels for (hidden_size, num_bins) {missing}: it is the --minimal build "
                f"(BUILD_VARIANT {build._variant()!r}).  Build the full library: python -m cnf_ot_amd.build --force",
                pytrace=False)
  yield
  if _WORST:
    print("\n[network shapes] worst error / bar per network, dim and kernel family:")
    for (net, D, fam), r in sorted(_WORST.items()):
      print(f"  {net:12s} D={D:<3d} {fam:14s} {r:.3f}")


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  return torch.device("cuda", 0)


def _cfgs(net, D, periodized=False):
  import oracle
  from cnf_ot_amd import FlowConfig
  kw = dict(num_layers=net.L, hidden_size=net.H, mlp_num_layers=net.M, num_bins=net.K)
  # (the C ABI carries the spline constants as float32: the oracle gets the same rounded values)
  okw = dict(D=D, L=net.L, H=net.H, M=net.M, K=net.K, min_bin_size=float(np.float32(1e-4)),
             min_knot_slope=float(np.float32(1e-4)))
  if periodized:
    return (FlowConfig.torus(dim=D, **kw),
            oracle.OracleConfig(range_min=0.0, range_max=float(np.float32(2 * np.pi)), periodized=True, **okw))
  return FlowConfig(dim=D, **kw), oracle.OracleConfig(**okw)


def _params(net, D, cfg, salt=0):
  """(float64 copy of float32 N(0, s^2) parameters, s)"""
  s = param_scale(net.H, net.M, D)
  rng = np.random.default_rng([net.H, net.K, net.M, net.L, D, salt])
  return rng.normal(0, s, cfg.param_count()).astype(np.float32).astype(np.float64), s


def _engine(cfg, p64, dev):
  from cnf_ot_amd import FlowEngine
  return FlowEngine(cfg, dev).load(torch.from_numpy(p64.astype(np.float32)).to(dev))


def _knobs(eng, fast=True, spl=1, mfma=0, dpar=0, precise=True):
  eng.set_pwl(0)
  eng.set_fast_math(fast)
  eng.set_samples_per_lane(spl)
  eng.set_mfma(mfma)
  eng.set_dpar(dpar)
  eng.set_precise(precise)


def _lp_factor(D, L):
  """The default network's log-density / log-det bars at this dim and depth (test_dim10_batch_vs_oracle,
  test_wave_per_dimension_kernel, test_wide_event_dimension, test_table_path_other_depths)."""
  return (1.0 if D <= 5 else 2.0 if D <= 10 else 5.0) * max(1.0, L / 2)


class _Case:
  """Collects every miss of one test case (so one run reports all of them) and the worst error per kernel family."""

  def __init__(self, name, net, D):
    self.name, self.net, self.D = name, net, D
    self.misses = []

  def check(self, family, what, err, bar, port=None, p999=None):
    """err: the kernel's errors against the float64 oracle; port: the float32 port's errors on the same inputs."""
    err = np.asarray(err, dtype=np.float64).reshape(-1)
    e = float(err.max()) if err.size else 0.0
    loose = LOOSENED.get((self.net.id, self.D, family, what))
    if loose is not None:
      bar, p999 = loose[0] or bar, loose[1] or p999
    key = (self.net.id, self.D, family)
    _WORST[key] = max(_WORST.get(key, 0.0), e / bar)
    ok = e <= bar
    msg = f"[{self.name} {family} {what}] max={e:.2e} bar={bar:.1e}"
    if p999 is not None:
      q = float(np.quantile(err, 0.999))
      ok = ok and q <= p999
      msg += f" p99.9={q:.2e} (bar {p999:.1e})"
    if port is not None and (loose is not None or not ok):
      ep = np.asarray(port, dtype=np.float64).reshape(-1)
      med, p99, pmed, pp99 = np.median(err), np.quantile(err, .99), np.median(ep), np.quantile(ep, .99)
      msg += (f" | kernel median={med:.2e} p99={p99:.2e} | fp32 port median={pmed:.2e} p99={pp99:.2e} "
              f"max={ep.max():.2e}")
      if loose is not None:       # a loosened case must stay within 2x of the port (the issue: beyond that, a bug)
        ok = ok and med <= 2 * pmed and p99 <= 2 * pp99
    print(msg)
    if not ok:
      self.misses.append(msg)

  def path(self, eng, want):
    got = eng.last_path()
    if got != want:
      self.misses.append(f"[{self.name}] last_path {got!r}, expected {want!r}")

  def done(self):
    assert not self.misses, "\n".join(self.misses)


# ---- flow passes ------------------------------------------------------------------------------------------------

BASE_VARIANTS = [     # name, knobs, expected path; mfma: hidden 16 / 5 bins only; dpar: dim >= 3 only
  ("mlp1", dict(spl=1), "mlp1"),
  ("mlp2", dict(spl=2), "mlp2"),
  ("ocml1", dict(fast=False, spl=1), "mlp1"),
  ("mfma1", dict(spl=1, mfma=1), "mfma"),
  ("mfma2", dict(spl=2, mfma=1), "mfma"),
  ("dpar1", dict(spl=1, dpar=2), "dpar"),
  ("dpar2", dict(spl=2, dpar=2), "dpar"),
]
INV_VARIANTS = [v for v in BASE_VARIANTS if not v[0].startswith("dpar")]


def _applies(name, net, D):
  if name.startswith("mfma"):
    return (net.H, net.K) == (16, 5)
  if name.startswith("dpar"):
    return D >= 3
  return True


def _flow_inputs(net, D):
  rng = np.random.default_rng([net.H, net.K, net.M, net.L, D, 1])
  noise = rng.normal(size=(B_MAIN, D)).astype(np.float32)
  if D == 2:                            # linear tails, where the default network's tests have them
    noise[0] = [11.0, -12.5]            # (at dim 5, a coordinate at 11 sigma feeds every later conditioner: the fp32
    noise[1] = [-11.5, 10.5]            #  port itself is then off by 1e-2)
  c = rng.uniform(0.0, 1.0, B_MAIN).astype(np.float32)            # per-sample conditions
  return noise, c


FLOW_CASES = [(net, D) for net in networks() for D in flow_dims(net)]


@pytest.mark.parametrize("net,D", FLOW_CASES, ids=[f"{n.id}-d{D}" for n, D in FLOW_CASES])
def test_flow_passes_vs_oracle(dev, net, D):
  """Both directions, every kernel variant that serves this shape, on a ragged batch with per-sample conditions and
  on B = 37 and B = 1 with one condition; the float64 kernels; seeded sampling == fill_normal + sample_logprob."""
  import oracle
  fcfg, ocfg = _cfgs(net, D)
  p64, s = _params(net, D, fcfg)
  print(f"\n[{net.id} D={D}] parameters N(0, {s}^2)")
  noise, c = _flow_inputs(net, D)
  n64, c64 = noise.astype(np.float64), c.astype(np.float64)
  # the oracle once per (network, dim, input), shared by every kernel variant below
  y_ref, fldj_ref = oracle.forward_logdet(ocfg, p64, n64, c64)
  lp_ref = oracle.sample_logprob(ocfg, p64, n64, c64)[1]
  y_in = y_ref.astype(np.float32)                  # data -> base on the oracle's (float32-rounded) samples
  xb_ref, ildj_ref = oracle.inverse_logdet(ocfg, p64, y_in.astype(np.float64), c64)
  lpd_ref = oracle.log_prob(ocfg, p64, y_in.astype(np.float64), c64)
  nb = max(B_SMALL)
  ys_ref, lps_ref = oracle.sample_logprob(ocfg, p64, n64[:nb], [C_SMALL])
  lpds_ref = oracle.log_prob(ocfg, p64, y_in[:nb].astype(np.float64), [C_SMALL])
  f = _lp_factor(D, net.L)
  case = _Case(f"{net.id} D={D}", net, D)
  eng = _engine(fcfg, p64, dev)
  x_d, c_d, y_d = _t(noise, dev), _t(c, dev), _t(y_in, dev)
  c1 = torch.tensor([C_SMALL], device=dev)
  # the oracle's own float32 port on the same inputs (_Case.check: LOOSENED cases, and the report of a miss)
  p32 = p64.astype(np.float32)
  P = dict(
    fwd=oracle.forward_logdet(ocfg, p32, noise, c, dtype=np.float32),
    lp=oracle.sample_logprob(ocfg, p32, noise, c, dtype=np.float32)[1],
    inv=oracle.inverse_logdet(ocfg, p32, y_in, c, dtype=np.float32),
    lpd=oracle.log_prob(ocfg, p32, y_in, c, dtype=np.float32),
    small=oracle.sample_logprob(ocfg, p32, noise[:nb], [C_SMALL], dtype=np.float32),
    small_lpd=oracle.log_prob(ocfg, p32, y_in[:nb], [C_SMALL], dtype=np.float32))
  pe = lambda a, ref: np.abs(np.asarray(a, dtype=np.float64) - ref)

  for name, kn, path in BASE_VARIANTS:
    if not _applies(name, net, D):
      continue
    _knobs(eng, **kn)
    fam = "base->data " + name
    y, fldj = eng.forward_logdet(x_d, c_d)
    case.path(eng, path)
    case.check(fam, "y", _err(y, y_ref), TOL_Y, port=pe(P["fwd"][0], y_ref))
    case.check(fam, "logdet", _err(fldj, fldj_ref), TOL_LD * f, port=pe(P["fwd"][1], fldj_ref))
    y2, lp = eng.sample_logprob(x_d, c_d)
    case.path(eng, path)
    if not torch.equal(y, y2):
      case.misses.append(f"[{case.name} {name}] sample_logprob's samples differ from forward_logdet's")
    case.check(fam, "log_prob", _err(lp, lp_ref), TOL_LP_SAMPLE * f, port=pe(P["lp"], lp_ref))
    for b in B_SMALL:
      ys, lps = eng.sample_logprob(x_d[:b].contiguous(), c1)
      case.path(eng, path)
      case.check(fam, f"y B={b}", _err(ys, ys_ref[:b]), TOL_Y, port=pe(P["small"][0][:b], ys_ref[:b]))
      case.check(fam, f"log_prob B={b}", _err(lps, lps_ref[:b]), TOL_LP_SAMPLE * f,
                 port=pe(P["small"][1][:b], lps_ref[:b]))
    # the base draw inside the kernel == cnf_fill_normal + the same kernel, bit for bit
    for b, cond in ((B_MAIN, c_d), (37, c1)):
      z = eng.normal(17, b, first_sample=5)
      ya, lpa = eng.sample_logprob(z, cond)
      yb, lpb = eng.sample_logprob_seeded(17, b, cond, first_sample=5)
      case.path(eng, path)
      if not (torch.equal(ya, yb) and torch.equal(lpa, lpb)):
        case.misses.append(f"[{case.name} {name}] seeded sampling differs from fill_normal + sample_logprob, B={b}")

  for name, kn, path in INV_VARIANTS:
    if not _applies(name, net, D):
      continue
    for precise in (True, False):
      _knobs(eng, precise=precise, **kn)
      fam = f"data->base {name}" + ("" if precise else " fp32")
      xb, ildj = eng.inverse_logdet(y_d, c_d)
      case.path(eng, path)
      if precise:
        case.check(fam, "x", _err(xb, xb_ref), TOL_Y, port=pe(P["inv"][0], xb_ref))
        case.check(fam, "logdet", _err(ildj, ildj_ref), TOL_LD * f, port=pe(P["inv"][1], ildj_ref))
      else:               # (the default network's tests hold plain fp32 positions to log_prob's bars only)
        case.check(fam, "x", _err(xb, xb_ref), TOL_X_FP32, port=pe(P["inv"][0], xb_ref))
        case.check(fam, "logdet", _err(ildj, ildj_ref), TOL_LP_FP32_MAX * f, port=pe(P["inv"][1], ildj_ref))
      lpd = eng.log_prob(y_d, c_d)
      case.path(eng, path)
      if precise:
        case.check(fam, "log_prob", _err(lpd, lpd_ref), TOL_LP_DATA_MAX * f, port=pe(P["lpd"], lpd_ref))
      else:
        case.check(fam, "log_prob", _err(lpd, lpd_ref), TOL_LP_FP32_MAX * f, port=pe(P["lpd"], lpd_ref),
                   p999=TOL_LP_FP32_P999 * f)
      for b in B_SMALL:
        lps = eng.log_prob(y_d[:b].contiguous(), c1)
        case.path(eng, path)
        case.check(fam, f"log_prob B={b}", _err(lps, lpds_ref[:b]), (TOL_LP_DATA_MAX if precise else TOL_LP_FP32_MAX) * f,
                   port=pe(P["small_lpd"][:b], lpds_ref[:b]))

  # float64 kernels (the reference's dtype)
  _knobs(eng)
  d64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)
  rel = lambda got, want: np.abs(got.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
  y, fldj = eng.forward_logdet(d64(n64), d64(c64))
  case.path(eng, "f64")
  _, lp = eng.sample_logprob(d64(n64), d64(c64))
  xb, ildj = eng.inverse_logdet(d64(y_in), d64(c64))
  lpd = eng.log_prob(d64(y_in), d64(c64))
  case.path(eng, "f64")
  for what, got, want in (("y", y, y_ref), ("logdet", fldj, fldj_ref), ("log_prob", lp, lp_ref), ("x", xb, xb_ref),
                          ("inverse logdet", ildj, ildj_ref), ("data log_prob", lpd, lpd_ref)):
    case.check("float64", what, rel(got, want), TOL_F64)
  eng.set_precise(True)
  case.done()


PERIODIC_NETS = networks()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("net", PERIODIC_NETS, ids=[n.id for n in PERIODIC_NETS])
def test_periodized_flow_vs_oracle(dev, net, D):
  """RQSFlow(periodized=True): sin / cos conditioner features, splines on [0, 2 pi] with circular slopes.  The bars
  of the default network's periodized test (test_gpu_parity.test_periodized_flow_vs_oracle)."""
  import oracle
  from cnf_ot_amd import FlowEngine, RQSFlow
  model = RQSFlow(event_shape=(D,), num_layers=net.L, hidden_sizes=[net.H] * net.M, num_bins=net.K, periodized=True)
  fcfg, ocfg = _cfgs(net, D, periodized=True)
  assert model.cfg == fcfg and oracle.param_count(ocfg) == fcfg.param_count()
  p64, s = _params(net, D, fcfg, salt=2)
  print(f"\n[{net.id} D={D} periodized] parameters N(0, {s}^2)")
  rng = np.random.default_rng([net.H, net.K, net.M, net.L, D, 3])
  B = B_MAIN + 1                                   # two slices
  x = rng.uniform(0.0, 2 * np.pi, size=(B, D)).astype(np.float32)
  x[0] = -0.5; x[1] = 2 * np.pi + 0.25; x[2] = 0.0            # linear tails and the boundary itself
  ts = np.array([0.3, 4.1])
  c_host = np.repeat(ts, B // 2)
  case = _Case(f"{net.id} D={D} periodized", net, D)
  eng = FlowEngine(fcfg, dev).load(torch.from_numpy(p64.astype(np.float32)).to(dev))
  eng.set_pwl(0)
  fam = "periodized"
  y, fldj = eng.forward_logdet(_t(x, dev), _t(ts, dev))
  case.path(eng, "mlp1")
  y_ref, fldj_ref = oracle.forward_logdet(ocfg, p64, x.astype(np.float64), c_host)
  case.check(fam, "y", _err(y, y_ref), TOL_Y)
  fl = max(1, D) * max(1.0, net.L / 2)
  case.check(fam, "logdet", _err(fldj, fldj_ref), TOL_LD * fl)
  y_in = y_ref.astype(np.float32)
  xb, ildj = eng.inverse_logdet(_t(y_in, dev), _t(ts, dev))
  case.path(eng, "mlp1")
  xb_ref, ildj_ref = oracle.inverse_logdet(ocfg, p64, y_in.astype(np.float64), c_host)
  case.check(fam, "x", _err(xb, xb_ref), TOL_Y)
  case.check(fam, "inverse logdet", _err(ildj, ildj_ref), TOL_LD * fl)
  lp = eng.log_prob(_t(y_in, dev), _t(ts, dev))
  case.path(eng, "mlp1")
  lp_ref = oracle.log_prob(ocfg, p64, y_in.astype(np.float64), c_host)
  case.check(fam, "log_prob", _err(lp, lp_ref), TOL_LP_FP32_MAX * fl)
  for b in B_SMALL:
    ys, _ = eng.forward_logdet(_t(x[:b], dev), torch.tensor([0.3], device=dev))
    case.path(eng, "mlp1")
    case.check(fam, f"y B={b}", _err(ys, y_ref[:b]), TOL_Y)      # (the first rows are in the t = 0.3 slice)
  yd, ld = eng.forward_logdet(torch.from_numpy(x.astype(np.float64)).to(dev), torch.from_numpy(ts).to(dev))
  case.path(eng, "f64")
  case.check("periodized float64", "y", _err(yd, y_ref), 1e-11)
  case.check("periodized float64", "logdet", _err(ld, fldj_ref), 1e-10)
  inside = (x > 0).all(1) & (x < 2 * np.pi).all(1)
  yi = y[torch.from_numpy(inside).to(dev)]
  assert yi.min().item() >= 0.0 and yi.max().item() <= 2 * np.pi + 1e-6
  case.done()


# ---- launches past the grid cap -------------------------------------------------------------------------------------

GRID_CASES = [      # kernel family, network, dim, knobs, samples per block
  ("mlp1", Net(64, 5, 3), 2, dict(spl=1), 256),
  ("mlp2", Net(16, 10, 3, 3), 5, dict(spl=2), 512),
  ("ocml1", Net(32, 8), 2, dict(fast=False, spl=1), 256),
  ("mfma1", Net(16, 5, 3), 2, dict(spl=1, mfma=1), 256),
  ("mfma2", Net(16, 5, 4), 5, dict(spl=2, mfma=1), 512),
  ("dpar1", Net(8, 5, 1), 17, dict(spl=1, dpar=2), 64),
  ("dpar2", Net(64, 5), 17, dict(spl=2, dpar=2), 128),
]


def _subset(B, ts, cap_rows):
  """A strided subset of the rows, the rows around the end of the first grid round and the whole last partial tile."""
  idx = np.concatenate([np.arange(0, B, 89), np.arange(max(0, cap_rows - 2 * ts), min(B, cap_rows + 2 * ts)),
                        np.arange((B - 1) // ts * ts - ts, B)])
  return np.unique(idx)


@pytest.mark.parametrize("fam,net,D,kn,ts", GRID_CASES, ids=[g[0] for g in GRID_CASES])
def test_launch_past_the_grid_cap(dev, fam, net, D, kn, ts):
  """More tiles than the num_cus * 8 blocks of the grid: every block strides over 1-2 tiles, the last one partial.
  The oracle on a strided subset, the first round's end and the last partial tile; then data -> base on the
  kernel's own samples (the precise path, the MLP or MFMA kernel of the same knobs)."""
  import oracle
  fcfg, ocfg = _cfgs(net, D)
  p64, s = _params(net, D, fcfg, salt=4)
  cap_rows = torch.cuda.get_device_properties(dev).multi_processor_count * 8 * ts
  B = cap_rows + cap_rows // 2 + 77
  print(f"\n[{net.id} D={D} {fam}] parameters N(0, {s}^2), B={B} (grid cap at {cap_rows} samples)")
  rng = np.random.default_rng([net.H, net.K, net.M, net.L, D, 5])
  noise = rng.normal(size=(B, D)).astype(np.float32)
  idx = _subset(B, ts, cap_rows)
  case = _Case(f"{net.id} D={D} grid cap", net, D)
  eng = _engine(fcfg, p64, dev)
  _knobs(eng, **kn)
  c = torch.tensor([0.61], device=dev)
  y, lp = eng.sample_logprob(_t(noise, dev), c)
  case.path(eng, {"ocml1": "mlp1", "mfma1": "mfma", "mfma2": "mfma", "dpar1": "dpar", "dpar2": "dpar"}.get(fam, fam))
  y_ref, lp_ref = oracle.sample_logprob(ocfg, p64, noise[idx].astype(np.float64), [0.61])
  f = _lp_factor(D, net.L)
  case.check(f"grid cap {fam}", "y", _err(y[torch.from_numpy(idx).to(dev)], y_ref), TOL_Y)
  case.check(f"grid cap {fam}", "log_prob", _err(lp[torch.from_numpy(idx).to(dev)], lp_ref), TOL_LP_SAMPLE * f)
  # data -> base: the same kernel, but the wave-per-dimension one exists for base -> data only
  inv_path = {"ocml1": "mlp1", "mfma1": "mfma", "mfma2": "mfma", "dpar1": "mlp1", "dpar2": "mlp2"}.get(fam, fam)
  lpd = eng.log_prob(y, c)
  case.path(eng, inv_path)
  yi = y[torch.from_numpy(idx).to(dev)].cpu().numpy().astype(np.float64)
  lpd_ref = oracle.log_prob(ocfg, p64, yi, [0.61])
  case.check(f"grid cap {fam}", "data log_prob", _err(lpd[torch.from_numpy(idx).to(dev)], lpd_ref), TOL_LP_DATA_MAX * f)
  case.done()


# ---- the fused loss kernel -------------------------------------------------------------------------------------------

LOSS_NETS = [Net(h, k) for h, k in kernel_configs()] + [Net(16, 5, 3), Net(64, 5, 1)]
LOSS_CASES = [(net, D) for net in LOSS_NETS for D in (2, 3)]
LOSS_VARIANTS = [("spl1", True, 1), ("spl2", True, 2), ("ocml", False, 1)]


def _rel_check(case, fam, name, got, want, rtol):
  got = float(got)
  rel = abs(got - want) / max(abs(want), 1e-12)
  print(f"[{case.name} {fam} {name}] gpu={got:.8g} oracle={want:.8g}")
  case.check(fam, name, rel, rtol)


@pytest.mark.parametrize("net,D", LOSS_CASES, ids=[f"{n.id}-d{D}" for n, D in LOSS_CASES])
def test_loss_terms_vs_oracle(dev, net, D):
  """The term set of test_gpu_losses.test_single_terms_dim2 through cnf_ot_amd.applications, at the dims where the
  reference defines each term, with one and two samples per lane and with ocml math, on a ragged batch; the density
  fit's neg_logprob term and both density-L2 kinds; seeded terms == tensor terms."""
  import oracle
  from oracle import losses as ol
  from cnf_ot_amd import FlowModel, Params, _capi, applications as app
  fcfg, ocfg = _cfgs(net, D)
  s = param_scale(net.H, net.M, D)
  model = FlowModel(fcfg)
  params = Params.random(fcfg, s, seed=net.H * 100 + net.K * 10 + net.M + D, device=dev)
  flow = ol.OracleFlow(ocfg, params.flat.cpu().double().numpy())
  print(f"\n[{net.id} D={D} losses] parameters N(0, {s}^2)")
  eng = model.engine(dev)
  B, seed, t = B_MAIN, 42, 0.4
  z = eng.normal(seed, B).cpu().double().numpy()
  comp = app.draw_components(seed, B)
  pts = (eng.normal(5, B) * 1.5 + 0.3).contiguous()          # data points of the density-fit term
  pts64 = pts.cpu().double().numpy()
  TS = [0.0, 0.3, 1.0]
  terms = []        # (name, gpu call, oracle value, relative bar)
  terms.append(("kinetic", lambda: app.kinetic_loss_fn(model, D, 0.01, params, t, seed, B),
                ol.kinetic_loss_fn(flow, D, 0.01, t, z), 2e-4))
  terms.append(("kinetic_score", lambda: app.kinetic_with_score_loss_fn(model, D, 2.0, 0.01, 0.01, params, t, seed, B),
                ol.kinetic_with_score_loss_fn(flow, D, 2.0, 0.01, 0.01, t, z), 2e-4))
  for sub in ("ou", "gradient", "nongradient") if D == 2 else ("ou", "lorenz"):
    terms.append((f"flow_matching[{sub}]",
                  functools.partial(app.flow_matching_loss_fn, model, D, 1.0, 0.5, sub, 0.01, 0.01, params, t, seed, B),
                  ol.flow_matching_loss_fn(flow, D, 1.0, 0.5, sub, t, z), 2e-4))
  for sub, a in (("quadratic", 0.0), ("double_well", 1.0), ("double_well", 0.5), ("obstacle", 0.0)):
    terms.append((f"potential[{sub},a={a}]", functools.partial(app.potential_loss_fn, model, D, a, sub, params, t, seed, B),
                  ol.potential_loss_fn(flow, a, sub, t, z), 2e-5))
  for c in (0.0, 0.3, 1.0):
    terms.append((f"reverse_kl[c={c}]", functools.partial(app.reverse_kl_loss_fn, model, D, 1.0, 4.0, params, c, seed, B),
                  ol.reverse_kl_loss_fn(flow, 1.0, 4.0, c, z), 5e-5))
  if D == 2:       # the mixture and the Gaussian source are 2-D
    for src in ("mixture", "gaussian"):
      for c in (0.0, 1.0):
        terms.append((f"kl[{src},c={c}]", functools.partial(app.kl_loss_fn, model, D, 1.0, params, c, seed, B, source=src),
                      ol.kl_loss_fn(flow, 1.0, c, z, src, comp), 2e-5))
  neg_lp = -flow.log_prob(pts64, [t]).sum()
  l2_base = []
  for tt in TS:
    y, lp = flow.sample_and_log_prob(z, [tt])
    l2_base.append(_want(np.exp(lp), _mix64(y, tt)))
  l2_data = [_want(np.exp(flow.log_prob(pts64, [tt])), _mix64(pts64, tt)) for tt in TS]
  nl_spec = app._spec(_capi.TERM_NEG_LOGPROB)
  l2_specs = [app._spec(k, coef=4.0, a=1.0, T=1.0) for k in (_capi.TERM_DENSITY_L2, _capi.TERM_DENSITY_L2_DATA)]
  zt = eng.normal(seed, B)
  case = _Case(f"{net.id} D={D} losses", net, D)
  for vname, fast, spl in LOSS_VARIANTS:
    eng.set_pwl(0)
    eng.set_fast_math(fast)
    eng.set_samples_per_lane(spl)
    fam = f"loss {vname}"
    for name, call, want, rtol in terms:
      got = call()
      case.path(eng, "loss_mlp")
      _rel_check(case, fam, name, got, want, rtol)
    _rel_check(case, fam, "neg_logprob", eng.loss_terms(nl_spec, pts, [t], B, True)[0], neg_lp, 2e-5)
    case.path(eng, "loss_mlp")
    for spec, what, inp, want in ((l2_specs[0], "density_l2", zt, l2_base), (l2_specs[1], "density_l2_data", pts, l2_data)):
      got = eng.loss_terms(spec, inp, TS, B, True).cpu().numpy()
      case.path(eng, "loss_mlp")
      for i, tt in enumerate(TS):
        w, sc = want[i]
        case.check(fam, f"{what} t={tt}", abs(float(got[i]) - w) / sc, TOL_L2)
    # seeded terms == tensor terms (test_gpu_losses.test_seeded_terms_equal_tensor_terms at this shape)
    Bs, S, first = 1000, 5, 777
    ts = np.linspace(0.1, 0.9, S).astype(np.float32)
    for spec in (app._spec(_capi.TERM_KINETIC, dt=0.01), app._spec(_capi.TERM_POTENTIAL, subtype=2),
                 app._spec(_capi.TERM_REVERSE_KL, T=1.0, beta=4.0)):
      own = torch.cat([eng.normal(9, Bs, first_sample=first + k * Bs) for k in range(S)])
      a = eng.loss_terms(spec, own, ts, Bs, False)
      b = eng.loss_terms_seeded(spec, 9, ts, Bs, first_sample=first, slice_stride=Bs)
      case.path(eng, "loss_mlp")
      if not torch.allclose(a, b, rtol=1e-12, atol=1e-9):
        case.misses.append(f"[{case.name} {vname}] seeded term {spec.kind} != tensor term: {a} vs {b}")
  eng.set_fast_math(True)
  eng.set_samples_per_lane(0)
  eng.set_pwl(1)
  case.done()


def test_loss_kernel_past_the_grid_cap(dev):
  """loss_kernel with more tiles than num_cus * 8 blocks, both lane widths, against the oracle on every sample."""
  from oracle import losses as ol
  from cnf_ot_amd import FlowModel, Params, _capi, applications as app
  net, D = Net(32, 8), 2
  fcfg, ocfg = _cfgs(net, D)
  s = param_scale(net.H, net.M, D)
  params = Params.random(fcfg, s, seed=77, device=dev)
  eng = FlowModel(fcfg).terms_backend(params)
  cap = torch.cuda.get_device_properties(dev).multi_processor_count * 8
  B = cap * 512 + cap * 128 + 77          # past the cap at two samples per lane; 2.5 rounds at one
  print(f"\n[{net.id} D={D} loss grid cap] parameters N(0, {s}^2), B={B}")
  z = eng.normal(3, B)
  z64 = z.cpu().double().numpy()
  flow = ol.OracleFlow(ocfg, params.flat.cpu().double().numpy())
  # per-slice sums: sum of v^2 over the B x D coordinates; sum of the potential over the B samples
  want = {"kinetic": ol.kinetic_loss_fn(flow, D, 0.01, 0.4, z64) * 2 / D * (B * D),
          "obstacle": ol.potential_loss_fn(flow, 0.0, "obstacle", 0.4, z64) * B}
  specs = {"kinetic": app._spec(_capi.TERM_KINETIC, dt=0.01), "obstacle": app._spec(_capi.TERM_POTENTIAL, subtype=2)}
  case = _Case(f"{net.id} D={D} loss grid cap", net, D)
  eng.set_pwl(0)
  for spl in (1, 2):
    eng.set_samples_per_lane(spl)
    for name, spec in specs.items():
      got = eng.loss_terms(spec, z, [0.4], B, True)[0]
      case.path(eng, "loss_mlp")
      _rel_check(case, f"loss grid cap spl{spl}", name, got, want[name], 2e-4 if name == "kinetic" else 2e-5)
  eng.set_samples_per_lane(0)
  eng.set_pwl(1)
  case.done()


def test_calc_kinetic_energy_at_a_wide_network(dev):
  """utils.calc_kinetic_energy (many slices per launch) at hidden 64, one MLP layer, dim 3."""
  from oracle import losses as ol
  from cnf_ot_amd import FlowModel, Params, utils as amd_utils
  net, D = Net(64, 5, 1), 3
  fcfg, ocfg = _cfgs(net, D)
  s = param_scale(net.H, net.M, D)
  model = FlowModel(fcfg)
  params = Params.random(fcfg, s, seed=8, device=dev)
  flow = ol.OracleFlow(ocfg, params.flat.cpu().double().numpy())
  be = model.terms_backend(params)
  Bs, S = 4096 + 5, 7
  draw = lambda k: be.normal(5, Bs, first_sample=k * Bs).cpu().double().numpy()
  got = amd_utils.calc_kinetic_energy(model.apply.sample, params, 5, batch_size=Bs, t_size=S, dim=D, slices_per_launch=3)
  case = _Case(f"{net.id} D={D} calc_kinetic_energy", net, D)
  case.path(model.engine(dev), "loss_mlp")
  _rel_check(case, "evaluator", "calc_kinetic_energy", got, ol.calc_kinetic_energy(flow, D, np.linspace(0, 1, S), draw),
             2e-4)
  case.done()


# ---- what these shapes must refuse ---------------------------------------------------------------------------------

OTHER_NETS = [n for n in networks() if n != DEFAULT]


@pytest.mark.parametrize("net", OTHER_NETS, ids=[n.id for n in OTHER_NETS])
def test_tables_fall_through_to_the_mlp_kernels(dev, net):
  """The conditioner tables exist for the default network only: dim 2, a uniform condition and set_pwl(2) must
  still run the MLP kernels at every other shape."""
  fcfg, _ = _cfgs(net, 2)
  p64, _ = _params(net, 2, fcfg, salt=6)
  eng = _engine(fcfg, p64, dev)
  eng.set_pwl(2)
  noise = np.random.default_rng(net.H + net.K).normal(size=(B_MAIN, 2)).astype(np.float32)
  ts = torch.tensor([0.2, 0.8], device=dev)          # two slices: the table path's own layout
  x = _t(noise[:B_MAIN - 1], dev)
  y, lp = eng.sample_logprob(x, ts)
  path = eng.last_path()
  assert path in ("mlp1", "mlp2", "mfma"), path
  lpd = eng.log_prob(y, ts)
  assert eng.last_path() in ("mlp1", "mlp2", "mfma"), eng.last_path()
  eng.set_pwl(0)          # the very kernels the MLP-only setting runs (their accuracy: test_flow_passes_vs_oracle)
  y0, lp0 = eng.sample_logprob(x, ts)
  assert eng.last_path() == path
  assert torch.equal(y, y0) and torch.equal(lp, lp0) and torch.equal(lpd, eng.log_prob(y, ts))
  eng.set_pwl(2)
  from cnf_ot_amd import _capi, applications as app
  eng.loss_terms(app._spec(_capi.TERM_KINETIC, dt=0.01), _t(noise, dev), [0.5], B_MAIN, True)
  assert eng.last_path() == "loss_mlp"
  eng.set_pwl(1)


@pytest.mark.parametrize("net", [Net(16, 5, 3), Net(32, 5), Net(16, 4)], ids=lambda n: n.id)
def test_gradient_entry_points_refuse_other_shapes(dev, net):
  """The backward kernels exist for hidden 16 / 2 MLP layers / 5 bins only: value_and_grad and a training step raise
  CnfError(CNF_ERR_UNSUPPORTED) and leave the parameters and the Adam state alone; the loss value still works."""
  from cnf_ot_amd import FlowModel, Params, _capi, applications as app, solvers
  fcfg, _ = _cfgs(net, 2)
  model = FlowModel(fcfg)
  params = Params.random(fcfg, param_scale(net.H, net.M, 2), seed=9, device=dev)
  before = params.flat.clone()
  vg = app.value_and_grad(functools.partial(app.kinetic_loss_fn, model, 2, 0.01))
  with pytest.raises(_capi.CnfError) as ei:
    vg(params, 0.5, 7, 256)
  assert ei.value.code == _capi.CNF_ERR_UNSUPPORTED
  opt = solvers.Adam(1e-3)
  state = opt.init(params)
  update = solvers.make_update(functools.partial(app.ot_loss_fn, model, 2, 1.0, 0.01, 4, "free"), opt, 256)
  with pytest.raises(_capi.CnfError) as ei:
    update(params, 7, 5000.0, state)
  assert ei.value.code == _capi.CNF_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert torch.equal(params.flat, before)
  assert state.step == 0 and not state.mu.any().item() and not state.nu.any().item()
  loss = app.ot_loss_fn(model, 2, 1.0, 0.01, 4, "free", params, 7, 5000.0, 256)
  assert np.isfinite(float(loss))
  assert np.isfinite(float(app.kinetic_loss_fn(model, 2, 0.01, params, 0.5, 7, 256)))
  assert torch.equal(params.flat, before)
