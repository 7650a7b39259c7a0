"""The table kernel's sampling direction after its instruction stream was shortened ("roots and
leftovers"): both splines form the inverse quadratic without scalings by literals, the `first` spline reads d0 bh
and 2 s from the prepared table, and the root's clip to [0, 1] is the clamp modifier of the packed product that
forms it (an asm statement behind v_rcp_f32, which carries its own wait state).

1. Oracle parity on the forced table path at the smallest shape that has the unmasked path, the tile step and a
   ragged tile: 3 slices of 4 098 samples (two full 2 048-tiles and a 2-sample one), t = 0, 0.45, 1.  Inputs are
   N(0, 1) draws with the specials of test_gpu_pwl_sampling_binsel.py merged in (+-10 exactly, floats either side,
   +-14), so waves hold tail lanes beside interior ones.  N(0, 0.2^2) is held to BASELINE.json's bars, N(0, 0.5^2)
   to the float32 port of the oracle on the same inputs (the rule of test_gpu_pwl_bench_shape.py).
2. The prepared table's new fields, through the spline (the header has no accessor): with the output layer of both
   conditioners zeroed every conditioned spline is the identity, and y is the `first` spline alone, applied once
   per coordinate -- whose quadratic is formed from the new fields.  `first` parameters at N(0, 1), seed 11: bins from 1.2
   to 8.1 wide and 0.6 to 7.6 high, knot slopes from 0.8 to 2.2.  Held to TOL_Y against the float64 oracle.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_pwl_bench_shape import TOL_LP, TOL_Y, _err

pytestmark = pytest.mark.gpu

SLICES, SLICE_LEN = 3, 4098
TS = np.array([0.0, 0.45, 1.0])
LO, HI = np.float32(-10.0), np.float32(10.0)


def _inputs():
  """[SLICES * SLICE_LEN, 2] float32: N(0, 1) draws, the specials spread over both coordinates of every slice."""
  ulp = np.spacing(np.float32(8.0))     # the float32 spacing on [8, 16): both sides of +-10
  j = np.arange(17, dtype=np.float32)
  b = np.arange(1, 5, dtype=np.float32)
  special = np.concatenate([HI - j * ulp, LO + j * ulp, HI + b * ulp, LO - b * ulp, np.float32([-14.0, 14.0])])
  rng = np.random.default_rng(7)
  x = rng.normal(size=(SLICES, SLICE_LEN, 2)).astype(np.float32)
  for s in range(SLICES):
    for coord in (0, 1):                # scattered: a special's wave neighbours are interior samples
      at = rng.choice(SLICE_LEN, special.size, replace=False)
      x[s, at, coord] = special
  return x.reshape(-1, 2)


def _sample(params):
  """(y, log_prob, y_ref, lp_ref) of one forced table-path launch on _inputs()."""
  import oracle
  from cnf_ot_amd import FlowEngine
  dev = params.flat.device
  eng = FlowEngine(params.cfg, dev).load(params)
  eng.set_pwl(2)
  noise = _inputs()
  y, lp = eng.sample_logprob(torch.from_numpy(noise).to(dev), torch.tensor(TS, dtype=torch.float32, device=dev))
  torch.cuda.synchronize()
  assert eng.last_path() == "tables"
  p64 = params.flat.cpu().double().numpy()
  c_host = np.repeat(TS.astype(np.float32).astype(np.float64), SLICE_LEN)
  y_ref, lp_ref = oracle.sample_logprob(oracle.OracleConfig(D=2), p64, noise.astype(np.float64), c_host)
  return y, lp, y_ref, lp_ref, p64, c_host, noise


@functools.lru_cache(maxsize=None)
def _run(scale):
  from cnf_ot_amd import FlowConfig, Params
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  cfg = FlowConfig(dim=2)
  return _sample(Params.random(cfg, scale, seed=42, device=torch.device("cuda", 0)))


@pytest.mark.parametrize("scale", [0.2, 0.5])
def test_ragged_table_launch_matches_oracle(scale):
  import oracle
  y, lp, y_ref, lp_ref, p64, c_host, noise = _run(scale)
  assert np.isfinite(y_ref).all() and np.isfinite(lp_ref).all()
  assert torch.isfinite(y).all() and torch.isfinite(lp).all()
  ey, elp = _err(y, y_ref), _err(lp, lp_ref)
  print(f"\n[sampling stream, N(0, {scale}^2)] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e} "
        f"median|dlogp|={np.median(elp):.2e} p99|dlogp|={np.quantile(elp, 0.99):.2e}")
  if scale <= 0.2:
    assert ey.max() <= TOL_Y
    assert elp.max() <= TOL_LP
  else:
    _, lp32 = oracle.sample_logprob(oracle.OracleConfig(D=2), p64.astype(np.float32), noise, c_host.astype(np.float32),
                                    dtype=np.float32)
    e_port = np.abs(lp32.astype(np.float64) - lp_ref)
    print(f"[fp32 C port] median|dlogp|={np.median(e_port):.2e} p99|dlogp|={np.quantile(e_port, 0.99):.2e} "
          f"max|dlogp|={e_port.max():.2e}")
    assert np.median(elp) <= 2 * np.median(e_port) + 1e-6
    assert np.quantile(elp, 0.99) <= 2 * np.quantile(e_port, 0.99) + 1e-5


def test_first_spline_alone_matches_oracle():
  """The new table fields (d0 bh, 2 s) through the only code that reads them."""
  from cnf_ot_amd import FlowConfig, Params
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  cfg = FlowConfig(dim=2)
  params = Params.random(cfg, 0.2, seed=42, device="cpu")
  first = np.random.default_rng(11).normal(0.0, 1.0, cfg.num_bijector_params).astype(np.float32)
  params["~"]["first"][:] = torch.from_numpy(first)
  for l in range(cfg.num_layers):
    for name in ("w", "b"):
      params[f"linear_out_layer{l}_d1"][name].zero_()
  y, lp, y_ref, lp_ref, _, _, noise = _sample(params.to(torch.device("cuda", 0)))
  assert np.isfinite(y_ref).all() and np.isfinite(lp_ref).all()
  # every conditioned spline is the identity: each coordinate went through `first` exactly once
  assert np.abs(y_ref - noise).max() > 0.5
  ey, elp = _err(y, y_ref), _err(lp, lp_ref)
  print(f"\n[`first` spline alone] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e}")
  assert ey.max() <= TOL_Y
