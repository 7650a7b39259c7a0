"""The dim-2 table kernel at the benchmark's own instantiation, against the float64 oracle.

bench.py times flow_pwl_kernel through the default dispatch (set_pwl(1)): full 2 048-sample tiles, the layer
count fixed at compile time (LFIX = 2), every table row in LDS.  The other table tests force the path at small,
ragged sizes, which run the same kernel with partial tiles.  Here the launch is bench-shaped (65 536 samples per
slice, every slice its own condition) and the dispatcher itself must pick the tables.

N(0, 0.2^2) (bench.py's parameters) is held to BASELINE.json's absolute bars.  N(0, 0.5^2) is the ill-conditioned
scale of the `wild` set (local slopes up to e^16): there log_prob is held to the bar of
test_wild_params_no_worse_than_fp32_port, the plain fp32 C port of the oracle on the same inputs.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLICES, SLICE_LEN = 32, 65536
TOL_Y = 2e-5                 # BASELINE.json's bars (tests/test_gpu_parity.py)
TOL_LP = 1e-5
RTOL = 2.5e-7                # ~2 fp32 ulps of the reference value (the representation floor of large values)


def _err(gpu, ref):
  d = np.abs(gpu.detach().cpu().numpy().astype(np.float64) - ref)
  return np.maximum(d - RTOL * np.abs(ref), 0.0)


@pytest.mark.parametrize("scale", [0.2, 0.5])
def test_bench_shaped_table_launch_matches_oracle(scale):
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  dev = torch.device("cuda", 0)
  cfg = FlowConfig(dim=2)
  ocfg = oracle.OracleConfig(D=2)
  params = Params.random(cfg, scale, seed=42, device=dev)     # scale 0.2: bench.py's parameters
  eng = FlowEngine(cfg, dev).load(params)
  noise = eng.normal(42, SLICES * SLICE_LEN)
  t = torch.linspace(0.0, 1.0, SLICES, device=dev)
  y, lp = eng.sample_logprob(noise, t)
  torch.cuda.synchronize()
  assert eng.last_path() == "tables"
  p64 = params.flat.cpu().double().numpy()
  c_host = np.repeat(t.cpu().double().numpy(), SLICE_LEN)
  y_ref, lp_ref = oracle.sample_logprob(ocfg, p64, noise.cpu().double().numpy(), c_host)
  ey, elp = _err(y, y_ref), _err(lp, lp_ref)
  print(f"\n[bench-shaped tables, N(0, {scale}^2)] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e} "
        f"median|dlogp|={np.median(elp):.2e} p99|dlogp|={np.quantile(elp, 0.99):.2e}")
  if scale <= 0.2:
    assert ey.max() <= TOL_Y
    assert elp.max() <= TOL_LP
  else:
    _, lp32 = oracle.sample_logprob(ocfg, p64.astype(np.float32), noise.cpu().numpy(), c_host.astype(np.float32),
                                    dtype=np.float32)
    e_port = np.abs(lp32.astype(np.float64) - lp_ref)
    print(f"[fp32 C port] median|dlogp|={np.median(e_port):.2e} p99|dlogp|={np.quantile(e_port, 0.99):.2e} "
          f"max|dlogp|={e_port.max():.2e}")
    assert np.median(elp) <= 2 * np.median(e_port) + 1e-6
    assert np.quantile(elp, 0.99) <= 2 * np.quantile(e_port, 0.99) + 1e-5
