"""applications._Ctx's noise cache on one rank, over the oracle backend (tests/oracle_backend.py): the cache holds
(draw, start, count) triples under integer keys AND the source samples -- one tensor -- under ("source", ...) keys, and a
call order the shipped losses do not use walks over both."""
import torch

from cnf_ot_amd import applications as app
from cnf_ot_amd.distributed import Shard
from cnf_ot_amd.params import FlowConfig, Params


def test_noise_after_a_source_draw_reuses_the_larger_draw(oracle_lib):
  """noise(256), the source entry of that draw (stored by _kl_sum, as the density-fit terms do), then noise(1024): the
  search for a larger draw meets the source entry, whose value is no triple; then noise(128) is the first 128 rows of
  the 1024 draw (one rank: a smaller draw is a prefix of the stream)."""
  from oracle_backend import OracleModel
  cfg = FlowConfig(dim=2)
  ctx = app._Ctx(OracleModel(cfg), Params.random(cfg, 0.2, seed=11), 42, Shard())
  z256, start, count = ctx.noise(256)
  assert (start, count) == (0, 256)
  app._kl_sum(ctx, 1.0, 0.0, 256, "gaussian", 1.0 / 256)
  assert torch.is_tensor(ctx._noise[("source", 256, "gaussian")])
  z1024, start, count = ctx.noise(1024)
  assert (start, count) == (0, 1024) and tuple(z1024.shape) == (1024, 2)
  z128, start, count = ctx.noise(128)
  assert (start, count) == (0, 128) and torch.equal(z128, z1024[:128])
  assert torch.equal(z256, z1024[:256])
