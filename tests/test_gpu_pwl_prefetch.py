"""The table flow kernel's prefetch ("Prefetch with no store wait"): the next tile's points are
requested with no wait on the stores of the tile before; a partial tile's masked loads are waited for where they are
issued, and the first tile's points in front of the loop.  That is no arithmetic: the bars are those of
test_gpu_pwl_bench_shape.py (TOL_Y, TOL_LP against the float64 oracle) on bench.py's parameter set, N(0, 0.2^2),
seed 42, the table path forced with set_pwl(2).  The shapes are the ones where the load paths differ (1-4); 5 was
written for two parts of the same change that were measured and not kept (the table search's cell clamp taken only
in waves whose tail test fired, the two samples' coordinates paired by packed moves) and stays as the check of the
search's far-out cells and of the coordinate pairing for whoever tries them again.

1. Blocks of one tile: 3 x 4 098 samples (9 tiles, 9 blocks) and 1 x 4 098: only the prologue's load runs.
2. A partial first tile: slices of 2 050 samples (one full tile and a 2-sample one), 5 tiles per block: every other
   block starts on a 2-sample tile, and every 2-sample tile inside a block is followed by the full tile of the next
   slice.  The grid is min(tiles, CUs), so the launch has 5 tiles per CU (640 slices on 256 CUs).  Both outputs, y
   alone and log|det| alone, into NaN-padded buffers.
3. The shared-points call (cnf_kinetic_potential_vjp's flow: 4 slices read ONE 4 098-sample slice) against the
   per-slice call, bit for bit.
4. The windowed instantiations: L = 4, 8 x 4 098, explicit noise against the oracle, the seeded call bitwise equal.
5. Far-out inputs (the cell clamp): 16 samples of a 4 096-sample slice, scattered over the waves, get +-9.9999, +-10,
   +-10.5, +-15.99, +-16, +-17, +-1e6, +-inf in one coordinate, the other, and both; against the MLP kernel and the
   oracle, and every other sample of the slice within the bars.  "Finite" is asked per sample (y and log_prob
   together): at +-inf the kernels agree that the sample's result is not finite and on nothing else (see the test).
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_pwl_bench_shape import RTOL, TOL_LP, TOL_Y, _err
from test_gpu_pwl_tile_loop import _bits, _pad_intact, _padded, _params64, _times

SLICE_LEN = 4098


def _engine(L=2):
  from cnf_ot_amd import FlowEngine
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  dev = torch.device("cuda", 0)
  cfg, params = _params64(L)
  eng = FlowEngine(cfg, dev).load(params.to(dev))
  eng.set_pwl(2)
  return eng, params, dev


@functools.lru_cache(maxsize=None)
def _launch(L, slices, slice_len):
  """One forced table-path launch for both outputs into padded buffers, and its float64 reference (shared)."""
  import oracle
  eng, params, dev = _engine(L)
  B = slices * slice_len
  noise = eng.normal(42, B)
  times = _times(slices)
  t = torch.from_numpy(times).to(dev)
  ybuf, lbuf = _padded(2 * B, dev), _padded(B, dev)
  y, lp = eng.sample_logprob(noise, t, out=ybuf[:2 * B].view(B, 2), logp_out=lbuf[:B])
  torch.cuda.synchronize()
  assert eng.last_path() == "tables"
  c_host = np.repeat(times.astype(np.float64), slice_len)
  y_ref, lp_ref = oracle.sample_logprob(oracle.OracleConfig(D=2, L=L), params.flat.double().numpy(),
                                        noise.cpu().double().numpy(), c_host)
  y_ref.setflags(write=False); lp_ref.setflags(write=False)
  return dict(eng=eng, noise=noise, t=t, y=y, lp=lp, ybuf=ybuf, lbuf=lbuf, y_ref=y_ref, lp_ref=lp_ref, B=B,
              params=params, c_host=c_host, L=L)


def _check(r, what):
  assert torch.isfinite(r["y"]).all() and torch.isfinite(r["lp"]).all()
  assert _pad_intact(r["ybuf"], 2 * r["B"]) and _pad_intact(r["lbuf"], r["B"])
  ey, elp = _err(r["y"], r["y_ref"]), _err(r["lp"], r["lp_ref"])
  print(f"\n[prefetch, {what}] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e}")
  assert ey.max() <= TOL_Y
  assert elp.max() <= TOL_LP


@pytest.mark.gpu
@pytest.mark.parametrize("slices", [3, 1])
def test_blocks_of_one_tile(slices):
  _check(_launch(2, slices, SLICE_LEN), f"{slices} x 4 098")


def _partial_first_slices():
  """Slices of 2 050 samples such that a block has 5 tiles (odd: every other block starts on a 2-sample tile)."""
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  return max(5, (5 * cus) // 2)


@pytest.mark.gpu
def test_partial_first_tile():
  import oracle
  n = _partial_first_slices()
  r = _launch(2, n, 2050)
  _check(r, f"{n} x 2 050, both outputs")
  eng, noise, t, B = r["eng"], r["noise"], r["t"], r["B"]
  dev = noise.device
  # y alone
  ybuf = _padded(2 * B, dev)
  y1, none = eng.sample_logprob(noise, t, want_logp=False, out=ybuf[:2 * B].view(B, 2))
  torch.cuda.synchronize()
  assert none is None and eng.last_path() == "tables"
  assert torch.equal(_bits(y1), _bits(r["y"])) and _pad_intact(ybuf, 2 * B)
  # log|det| alone: `out` null in the sampling direction
  lbuf = _padded(B, dev)
  none, ld = eng._run(eng.lib.cnf_forward_logdet, "cnf_forward_logdet", noise, t, False, True, aux=lbuf[:B])
  torch.cuda.synchronize()
  assert none is None and eng.last_path() == "tables" and _pad_intact(lbuf, B)
  _, ld_ref = oracle.forward_logdet(oracle.OracleConfig(D=2), r["params"].flat.double().numpy(),
                                    noise.cpu().double().numpy(), r["c_host"])
  eld = _err(ld, ld_ref)
  print(f"[prefetch, {n} x 2 050, log|det| alone] max|dlogdet|={eld.max():.2e}")
  assert torch.isfinite(ld).all() and eld.max() <= TOL_LP


@pytest.mark.gpu
def test_shared_points_call():
  """cnf_kinetic_potential_vjp pushes ONE draw to every condition: its flow launch reads the same 4 098 points in each
  of the 4 slices (S = 2 times, t -+ dt/2) and leaves the positions at the head of the work buffer."""
  eng, _, dev = _engine(2)
  count, S, dt = SLICE_LEN, 2, 0.05
  z = eng.normal(42, count)
  tm = np.array([0.3, 0.7], dtype=np.float32)
  conds = torch.from_numpy(np.concatenate([tm - np.float32(0.5 * dt), tm + np.float32(0.5 * dt)])).to(dev)
  done = eng.kinetic_potential_vjp(z, conds, S, dt, 1.0, None)
  torch.cuda.synchronize()
  assert done is not None, "the shared-points call did not take the table route"
  ns = 2 * S
  shared = eng._kp_work[:2 * ns * count].clone().view(ns * count, 2)
  y, none = eng.sample_logprob(z.repeat(ns, 1), conds, want_logp=False)
  torch.cuda.synchronize()
  assert none is None and eng.last_path() == "tables"
  assert torch.isfinite(shared).all()
  assert torch.equal(_bits(shared), _bits(y))
  # the slices differ (each has its own condition): the comparison is not one slice against itself
  assert not torch.equal(_bits(shared[:count]), _bits(shared[count:2 * count]))


@pytest.mark.gpu
def test_windowed_instantiation():
  r = _launch(4, 8, SLICE_LEN)
  _check(r, "L = 4, 8 x 4 098")
  B, dev = r["B"], r["noise"].device
  ybuf, lbuf = _padded(2 * B, dev), _padded(B, dev)
  y, lp = r["eng"].sample_logprob_seeded(42, B, r["t"], out=ybuf[:2 * B].view(B, 2), logp_out=lbuf[:B])
  torch.cuda.synchronize()
  assert r["eng"].last_path() == "tables"
  assert torch.equal(_bits(y), _bits(r["y"])) and torch.equal(_bits(lp), _bits(r["lp"]))
  assert _pad_intact(ybuf, 2 * B) and _pad_intact(lbuf, B)


FAR = np.array([s * v for v in (9.9999, 10.0, 10.5, 15.99, 16.0, 17.0, 1e6, np.inf) for s in (1.0, -1.0)], dtype=np.float32)
# 16 samples over 9 of the slice's 32 waves (a wave holds 128 consecutive samples); (130, 131) share a lane
FAR_AT = np.array([5, 6, 130, 131, 300, 777, 1023, 1024, 1500, 2047, 2048, 2500, 3000, 3333, 4000, 4095])


def _err_against(a, b):
  """|a - b| beyond the representation floor of b (the bars' own RTOL), both float32 tensors."""
  a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
  return np.maximum(np.abs(a - b) - RTOL * np.abs(b), 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("coords", [(0,), (1,), (0, 1)])
def test_far_inputs(coords):
  import oracle
  eng, params, dev = _engine(2)
  B = 4096
  noise = eng.normal(42, B).clone()
  for d in coords:
    noise[torch.from_numpy(FAR_AT).to(dev), d] = torch.from_numpy(FAR).to(dev)
  t = torch.tensor([0.5], device=dev)
  y, lp = eng.sample_logprob(noise, t)
  torch.cuda.synchronize()
  assert eng.last_path() == "tables"
  eng.set_pwl(0)
  ym, lpm = eng.sample_logprob(noise, t)
  torch.cuda.synchronize()
  assert eng.last_path() != "tables"
  # the MLP kernel on the same inputs: the same samples have a finite result (y and log_prob), and those are within
  # the bars.  Finiteness is taken per sample, not per element: at +-inf no kernel has a defined answer for the parts
  # (the oracle: y = (inf, 2.115), log_prob = -inf; the MLP kernel (nan, 2.115), -inf; the table kernel (nan, -10), nan,
  # before this change and after it), so only "this sample's result is not finite" can be asked of both.
  fm = (torch.isfinite(ym).all(dim=1) & torch.isfinite(lpm)).cpu().numpy()
  ft = (torch.isfinite(y).all(dim=1) & torch.isfinite(lp)).cpu().numpy()
  assert np.array_equal(ft, fm)
  assert fm.sum() == B - 2
  fy = fl = fm
  ey, elp = _err_against(y, ym)[fm], _err_against(lp, lpm)[fm]
  print(f"\n[far inputs, coordinates {coords}] against the MLP kernel: max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e}")
  assert ey.max() <= TOL_Y
  assert elp.max() <= TOL_LP
  # the float64 oracle where the input is finite (every untouched sample of the touched waves among them)
  fin = torch.isfinite(noise).all(dim=1).cpu().numpy()
  assert fin.sum() == B - 2
  with np.errstate(all="ignore"):
    y_ref, lp_ref = oracle.sample_logprob(oracle.OracleConfig(D=2), params.flat.double().numpy(),
                                          noise.cpu().double().numpy()[fin], np.full(int(fin.sum()), 0.5))
  assert fy[fin].all() and fl[fin].all()
  oy, olp = _err(y[torch.from_numpy(fin).to(dev)], y_ref), _err(lp[torch.from_numpy(fin).to(dev)], lp_ref)
  print(f"[far inputs, coordinates {coords}] against the oracle: max|dy|={oy.max():.2e} max|dlogp|={olp.max():.2e}")
  assert oy.max() <= TOL_Y
  assert olp.max() <= TOL_LP
