"""CPU checks of every network shape the engine compiles (tests/network_shapes.py): the host, the C library and the
oracle agree on the parameter layout, parameters survive an npz round trip, and the library supports exactly the
(hidden_size, num_bins) pairs of CNF_KERNEL_CONFIGS.  No compute calls."""
import numpy as np
import pytest
import torch

from network_shapes import flow_dims, kernel_configs, networks

from cnf_ot_amd import _capi
from cnf_ot_amd.flows import _c_config
from cnf_ot_amd.params import FlowConfig, Params, param_spec

CASES = [(net, D, per) for net in networks() for D in sorted(set(flow_dims(net)) | {3}) for per in (False, True)]


@pytest.mark.parametrize("net,D,periodized", CASES, ids=[f"{n.id}-d{D}{'-torus' if p else ''}" for n, D, p in CASES])
def test_param_counts_agree(oracle_lib, net, D, periodized):
  kw = dict(num_layers=net.L, hidden_size=net.H, mlp_num_layers=net.M, num_bins=net.K)
  cfg = FlowConfig.torus(dim=D, **kw) if periodized else FlowConfig(dim=D, **kw)
  ocfg = oracle_lib.OracleConfig(D=D, L=net.L, H=net.H, M=net.M, K=net.K, periodized=periodized)
  n = cfg.param_count()
  assert _capi.lib().cnf_param_count(_c_config(cfg)) == n
  assert oracle_lib.param_count(ocfg) == n
  assert sum(int(np.prod(s)) for _, _, s in param_spec(cfg)) == n


@pytest.mark.parametrize("net", networks(), ids=lambda n: n.id)
def test_params_npz_round_trip_keeps_every_leaf(tmp_path, net):
  cfg = FlowConfig(dim=5, num_layers=net.L, hidden_size=net.H, mlp_num_layers=net.M, num_bins=net.K)
  p = Params.random(cfg, 0.3, seed=net.H + net.K)
  path = str(tmp_path / "p.npz")
  p.save_npz(path)
  with np.load(path) as z:
    assert sorted(z.files) == sorted(f"{m}/{n}" for m, n, _ in param_spec(cfg))
  q = Params.load_npz(cfg, path)
  assert torch.equal(p.flat, q.flat)
  for (m, n, a), (_, _, b) in zip(p.leaves(), q.leaves()):
    assert torch.equal(a, b), (m, n)


def test_library_supports_exactly_the_compiled_pairs():
  pairs = set(kernel_configs())
  assert (16, 5) in pairs, pairs
  lib = _capi.lib()
  cfg = _capi.CnfConfig()
  lib.cnf_config_default(cfg, 2)
  hs = sorted({h for h, _ in pairs} | {1, 4, 12, 17, 24, 48, 128})
  ks = sorted({k for _, k in pairs} | {1, 3, 6, 7, 9, 11, 16})
  got = set()
  for h in hs:
    for k in ks:
      cfg.hidden_size, cfg.num_bins = h, k
      if lib.cnf_config_supported(cfg):
        got.add((h, k))
  assert got == pairs, (f"supported {sorted(got)} != CNF_KERNEL_CONFIGS {sorted(pairs)}"
                        + (" (a --minimal build: rebuild with python -m cnf_ot_amd.build --force)" if got == {(16, 5)} else ""))
  for m in (1, 3, 16):           # the depth is a run-time loop: any mlp_num_layers up to 16
    cfg.hidden_size, cfg.num_bins, cfg.mlp_num_layers = 32, 8, m
    assert lib.cnf_config_supported(cfg) == 1
  cfg.mlp_num_layers = 17
  assert lib.cnf_config_supported(cfg) == 0
