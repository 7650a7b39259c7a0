"""The table flow kernel's tile loop ("the tile loop"): the next tile's points are taken in front of
this tile's stores, a full tile of a call for both outputs stores without forming lane validity, and within a slice the
tile geometry is stepped in 32 bits.  None of that is arithmetic, so the bars are those of
test_gpu_pwl_bench_shape.py (TOL_Y, TOL_LP against the float64 oracle) on bench.py's parameter set, N(0, 0.2^2),
seed 42; what is new here is which blocks, tiles and store paths the shapes reach.

1. Hand-overs inside a block, starting mid-slice: 643 slices of 4 098 samples (two full 2 048-tiles and a 2-sample
   one): 1 929 tiles, about 8 per block on 256 CUs, so a block walks three slices, begins in the middle of one and
   meets ragged tiles in mid-range.  A block that kept the previous slice's tables must fail: at t = linspace(0, 1,
   643) neighbouring slices' reference outputs differ by as little as 1.4e-3 in y and 5.2e-4 in log_prob at the probe
   points (measured on the oracle), under 100 x the bars, so the same 643 times are visited four grid steps apart
   (t_i = grid[4 i mod 643]); the oracle-only test asserts the separation.
2. Every store path of that launch: both outputs, y alone, log|det| beside y and alone (cnf_forward_logdet, the
   sampling direction's call with `out` null), log_prob alone (cnf_log_prob: data -> base, `out` null), and the
   seeded entry point bitwise equal to explicit noise.  Outputs live in buffers 64 elements longer than needed,
   pre-filled with a NaN of a fixed payload that must survive.
3. Ragged shapes in one slice: 4 097 samples (a one-sample tile: only a lane's first sample exists) and 2.
4. The windowed instantiations (L = 4: the first 112 rows of each table in LDS), the shape of 1 cut to 40 slices:
   explicit noise against the oracle, and the seeded one (the kernel with the fewest registers to spare) bitwise
   equal to it.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_pwl_bench_shape import TOL_LP, TOL_Y, _err

SLICES, SLICE_LEN = 643, 4098
PAD = 64
PAYLOAD = 0x7FC0BEEF                     # a quiet NaN no kernel produces


def _times(n=SLICES):
  """The grid linspace(0, 1, 643), neighbours four grid steps apart (the first n of them)."""
  grid = np.linspace(0.0, 1.0, SLICES).astype(np.float32)
  return grid[(4 * np.arange(n)) % SLICES]


def _params64(L=2):
  from cnf_ot_amd import FlowConfig, Params
  cfg = FlowConfig(dim=2, num_layers=L)
  return cfg, Params.random(cfg, 0.2, seed=42, device="cpu")


@pytest.mark.parametrize("L", [2, 4])
def test_neighbouring_slices_differ_on_the_oracle(L):
  """CPU only: a stale table (the previous slice's) would move the outputs by more than 100 x the bars."""
  import oracle
  _, params = _params64(L)
  n = SLICES if L == 2 else 40
  t = _times(n).astype(np.float64)
  probe = np.random.default_rng(5).normal(size=(16, 2))
  y, lp = oracle.sample_logprob(oracle.OracleConfig(D=2, L=L), params.flat.double().numpy(), np.tile(probe, (n, 1)),
                                np.repeat(t, 16))
  dy = np.abs(np.diff(y.reshape(n, 16, 2), axis=0)).max(axis=(1, 2))
  dlp = np.abs(np.diff(lp.reshape(n, 16), axis=0)).max(axis=1)
  print(f"\n[neighbouring slices, L={L}] min max|dy|={dy.min():.2e} min max|dlogp|={dlp.min():.2e}")
  assert dy.min() > 100 * TOL_Y
  assert dlp.min() > 100 * TOL_LP


def _padded(n, dev):
  """A float32 buffer of n + PAD elements, every one the payload NaN."""
  return torch.full((n + PAD,), PAYLOAD, dtype=torch.int32, device=dev).view(torch.float32)


def _pad_intact(buf, n):
  return bool((buf.view(torch.int32)[n:] == PAYLOAD).all().item())


def _bits(t):
  return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _launch(L, slices, slice_len):
  """One forced table-path launch for both outputs into padded buffers, and its float64 reference (shared)."""
  import oracle
  from cnf_ot_amd import FlowEngine
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  dev = torch.device("cuda", 0)
  cfg, params = _params64(L)
  eng = FlowEngine(cfg, dev).load(params.to(dev))
  eng.set_pwl(2)
  B = slices * slice_len
  noise = eng.normal(42, B)
  t = torch.from_numpy(_times(slices)).to(dev)
  ybuf, lbuf = _padded(2 * B, dev), _padded(B, dev)
  y, lp = eng.sample_logprob(noise, t, out=ybuf[:2 * B].view(B, 2), logp_out=lbuf[:B])
  torch.cuda.synchronize()
  assert eng.last_path() == "tables"
  c_host = np.repeat(_times(slices).astype(np.float64), slice_len)
  y_ref, lp_ref = oracle.sample_logprob(oracle.OracleConfig(D=2, L=L), params.flat.double().numpy(),
                                        noise.cpu().double().numpy(), c_host)
  y_ref.setflags(write=False); lp_ref.setflags(write=False)
  return dict(eng=eng, noise=noise, t=t, y=y, lp=lp, ybuf=ybuf, lbuf=lbuf, y_ref=y_ref, lp_ref=lp_ref, B=B,
              params=params, c_host=c_host)


def _check(r, what):
  assert torch.isfinite(r["y"]).all() and torch.isfinite(r["lp"]).all()
  assert _pad_intact(r["ybuf"], 2 * r["B"]) and _pad_intact(r["lbuf"], r["B"])
  ey, elp = _err(r["y"], r["y_ref"]), _err(r["lp"], r["lp_ref"])
  print(f"\n[tile loop, {what}] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e}")
  assert ey.max() <= TOL_Y
  assert elp.max() <= TOL_LP


@pytest.mark.gpu
def test_handovers_inside_a_block():
  _check(_launch(2, SLICES, SLICE_LEN), "643 x 4 098")


@pytest.mark.gpu
def test_every_store_path():
  import oracle
  r = _launch(2, SLICES, SLICE_LEN)
  _check(r, "643 x 4 098, both outputs")
  eng, noise, t, B = r["eng"], r["noise"], r["t"], r["B"]
  dev = noise.device
  # y alone
  ybuf = _padded(2 * B, dev)
  y1, none = eng.sample_logprob(noise, t, want_logp=False, out=ybuf[:2 * B].view(B, 2))
  assert none is None and eng.last_path() == "tables"
  assert torch.equal(_bits(y1), _bits(r["y"])) and _pad_intact(ybuf, 2 * B)
  # y and log|det| (the other meaning of aux), against the oracle; log_prob = base - log|det| ties it to the first launch
  lbuf = _padded(B, dev)
  y2, ld = eng._run(eng.lib.cnf_forward_logdet, "cnf_forward_logdet", noise, t, True, True,
                    out=ybuf[:2 * B].view(B, 2), aux=lbuf[:B])
  assert eng.last_path() == "tables"
  assert torch.equal(_bits(y2), _bits(r["y"])) and _pad_intact(ybuf, 2 * B) and _pad_intact(lbuf, B)
  _, ld_ref = oracle.forward_logdet(oracle.OracleConfig(D=2), r["params"].flat.double().numpy(),
                                    noise.cpu().double().numpy(), r["c_host"])
  eld = _err(ld, ld_ref)
  print(f"\n[tile loop, log|det|] max|dlogdet|={eld.max():.2e}")
  assert torch.isfinite(ld).all() and eld.max() <= TOL_LP
  # log|det| alone: `out` null in the sampling direction
  lbuf2 = _padded(B, dev)
  none, ld2 = eng._run(eng.lib.cnf_forward_logdet, "cnf_forward_logdet", noise, t, False, True, aux=lbuf2[:B])
  assert none is None and eng.last_path() == "tables"
  assert torch.equal(_bits(ld2), _bits(ld)) and _pad_intact(lbuf2, B)
  # log_prob alone, data -> base (`out` null): the density of the samples just drawn
  # (FlowEngine.log_prob allocates its result itself: the same C call, into a padded buffer)
  from cnf_ot_amd import _capi
  from cnf_ot_amd.flows import _OnDevice, _stream_ptr
  lbuf3 = _padded(B, dev)
  lp3 = lbuf3[:B]
  c, c_block = eng.cond(t, B, torch.float32)
  with _OnDevice(dev):
    _capi.check(eng.lib.cnf_log_prob(eng._h, r["y"].data_ptr(), c.data_ptr(), c_block, lp3.data_ptr(), B,
                                     _stream_ptr(dev)), "cnf_log_prob")
  torch.cuda.synchronize()
  assert eng.last_path() == "tables" and _pad_intact(lbuf3, B)
  assert torch.equal(_bits(eng.log_prob(r["y"], t)), _bits(lp3))
  lp3_ref = oracle.log_prob(oracle.OracleConfig(D=2), r["params"].flat.double().numpy(),
                            r["y"].cpu().double().numpy(), r["c_host"])
  e3 = _err(lp3, lp3_ref)
  print(f"[tile loop, log_prob alone] max|dlogp|={e3.max():.2e}")
  assert torch.isfinite(lp3).all() and e3.max() <= TOL_LP
  # the seeded entry point on the same stream
  ybuf4, lbuf4 = _padded(2 * B, dev), _padded(B, dev)
  y4, lp4 = eng.sample_logprob_seeded(42, B, t, out=ybuf4[:2 * B].view(B, 2), logp_out=lbuf4[:B])
  torch.cuda.synchronize()
  assert eng.last_path() == "tables"
  assert torch.equal(_bits(y4), _bits(r["y"])) and torch.equal(_bits(lp4), _bits(r["lp"]))
  assert _pad_intact(ybuf4, 2 * B) and _pad_intact(lbuf4, B)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [4097, 2])
def test_ragged_single_slice(B):
  r = _launch(2, 1, B)
  _check(r, f"1 x {B}")
  eng = r["eng"]
  dev = r["noise"].device
  ybuf, lbuf = _padded(2 * B, dev), _padded(B, dev)
  y, lp = eng.sample_logprob_seeded(42, B, r["t"], out=ybuf[:2 * B].view(B, 2), logp_out=lbuf[:B])
  torch.cuda.synchronize()
  assert torch.equal(_bits(y), _bits(r["y"])) and torch.equal(_bits(lp), _bits(r["lp"]))
  assert _pad_intact(ybuf, 2 * B) and _pad_intact(lbuf, B)


@pytest.mark.gpu
def test_windowed_instantiation():
  r = _launch(4, 40, SLICE_LEN)
  _check(r, "L = 4, 40 x 4 098")
  B, dev = r["B"], r["noise"].device
  ybuf, lbuf = _padded(2 * B, dev), _padded(B, dev)
  y, lp = r["eng"].sample_logprob_seeded(42, B, r["t"], out=ybuf[:2 * B].view(B, 2), logp_out=lbuf[:B])
  torch.cuda.synchronize()
  assert r["eng"].last_path() == "tables"
  assert torch.equal(_bits(y), _bits(r["y"])) and torch.equal(_bits(lp), _bits(r["lp"]))
  assert _pad_intact(ybuf, 2 * B) and _pad_intact(lbuf, B)
