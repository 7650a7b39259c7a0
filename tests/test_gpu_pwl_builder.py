"""The two builders of the dim-2 conditioner tables write the same bytes.

`pwl_build_kernel` (512 threads per table) is the reference; `pwl_build_lean_kernel` (one wave per table) must
reproduce every float and every grid entry bit for bit: that is what lets `build_tables()` choose between them by
table count.  The tables are read through `FlowEngine.build_tables`
(cnf_internal_build_tables_into), into buffers pre-filled with a pattern, so what neither builder writes -- the rows
past the last piece, the rows' padding -- compares equal too and a stray write of either does not.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# cnf_pwl.h
NBP, NG, NREF, ROW, NPIECE = 320, 2048, 304, 36, 289
OFF_GRID, OFF_REF, OFF_PIECE = NBP, NBP + NG // 2, NBP + NG // 2 + NREF
TBL = OFF_PIECE + NPIECE * ROW
REFERENCE, LEAN = 1, 2
# build_tables() (cnf_flow.hip): the lean builder from this many tables up
LEAN_MIN_TABLES = 2048
FILL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  return torch.device("cuda", 0)


def _engine(L, params, dev):
  from cnf_ot_amd import FlowConfig, FlowEngine
  eng = FlowEngine(FlowConfig(dim=2, num_layers=L, hidden_size=16, mlp_num_layers=2, num_bins=5), dev)
  eng.load(torch.from_numpy(np.asarray(params, dtype=np.float32)).to(dev))
  return eng


def _layer(params, l):
  """W0[c row | u row] 32, b0 16, W1 256, b1 16, Wout 256, bout 16 of flow layer l (a view)"""
  return params[16 + 592 * l: 16 + 592 * (l + 1)]


def _params(kind, L):
  rng = np.random.default_rng(11)
  n = 16 + 592 * L
  p = np.zeros(n)
  if kind == "zeros":
    pass
  elif kind == "first_only":
    p[:16] = rng.normal(0, 0.5, 16)
  elif kind == "random":
    p = rng.normal(0, 0.2, n)
  elif kind == "zigzag":          # second-layer units cross zero in every first-layer interval: ~256 pieces
    p[:16] = rng.normal(0, 0.3, 16)
    for l in range(L):
      w = _layer(p, l)
      w[16:32] = 1.0
      w[32:48] = -np.linspace(-7.5, 7.5, 16)
      slopes = np.array([1.0] + [-2.0, 2.0] * 7 + [-2.0])
      w[48:304] = (slopes[:, None] * (1.0 + 0.01 * np.arange(16))[None, :]).reshape(-1)
      w[304:320] = -0.5 + 0.02 * (np.arange(16) - 8)
      w[320:576] = rng.normal(0, 0.3, 256)
      w[576:592] = rng.normal(0, 0.3, 16)
  elif kind == "wide_pieces":     # breakpoints at |u| ~ 1e3
    p = rng.normal(0, 0.2, n)
    for l in range(L):
      _layer(p, l)[16:24] *= 1e-3
  elif kind == "ties":            # two first-layer units with the same breakpoint, one that does not depend on u
    p = rng.normal(0, 0.2, n)
    for l in range(L):
      w = _layer(p, l)
      w[1], w[17], w[33] = w[0], w[16], w[32]
      w[18] = 0.0
  elif kind in ("pieces16", "pieces17"):
    # No second-layer root (W1 >= 0 and b1 > 0: every second-layer unit is positive everywhere), so the pieces are
    # the first-layer intervals: 17, or 16 with one unit independent of u.  16 is a multiple of the 4 pieces the lean
    # builder takes per pass; 17 is one more.
    p = rng.normal(0, 0.2, n)
    for l in range(L):
      w = _layer(p, l)
      w[16:32] = np.where(np.abs(w[16:32]) < 0.05, 0.1, w[16:32])
      w[48:304] = np.abs(w[48:304])
      w[304:320] = 0.5 + np.abs(w[304:320])
      if kind == "pieces16":
        w[16 + 5] = 0.0
  else:
    raise ValueError(kind)
  return p.astype(np.float32)


def _build(eng, mode, c, c_offset):
  out = torch.full((c.numel(), eng.cfg.num_layers, TBL), FILL, dtype=torch.int32, device=c.device).view(torch.float32)
  eng.set_pwl_builder(mode)
  eng.build_tables(c, c_offset, out=out)
  assert eng.last_pwl_builder() == mode
  return out.view(torch.int32)


KINDS = ["zeros", "first_only", "random", "zigzag", "wide_pieces", "ties", "pieces16", "pieces17"]


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_lean_builder_writes_the_reference_bytes(dev, kind, L):
  """1, 5 and 67 conditions, with a non-zero c_offset: bp[] with its NaN padding and the count slot, the whole grid,
  ref[0 .. n] and rows 0 .. n with their u_ref slot, as bit patterns -- and everything else untouched."""
  eng = _engine(L, _params(kind, L), dev)
  rng = np.random.default_rng(5)
  for n_cond, c_offset in ((1, 0.0), (5, -0.03125), (67, 0.0123)):
    c = torch.from_numpy(rng.uniform(0.0, 1.0, n_cond).astype(np.float32)).to(dev)
    ref = _build(eng, REFERENCE, c, c_offset)
    n = ref[:, :, NBP - 1]                                    # pieces 0 .. n
    assert int(n.min()) >= 0 and int(n.max()) <= NPIECE - 1
    pieces = n + 1
    if kind in ("zeros", "first_only"):
      assert int(pieces.max()) == 1
    elif kind == "zigzag":
      assert int(pieces.min()) > 200
    elif kind == "pieces16":
      assert int(pieces.min()) == 16 and int(pieces.max()) == 16
    elif kind == "pieces17":
      assert int(pieces.min()) == 17 and int(pieces.max()) == 17
    # the reference wrote what the comparison is meant to cover, and nothing past it
    in_use = torch.arange(NPIECE, device=dev)[None, None, :] <= n[:, :, None]
    head = torch.ones((n_cond, L, OFF_REF), dtype=torch.bool, device=dev)
    refs = torch.zeros((n_cond, L, NREF), dtype=torch.bool, device=dev)
    refs[:, :, :NPIECE] = in_use
    rows = torch.zeros((n_cond, L, NPIECE, ROW), dtype=torch.bool, device=dev)
    rows[:, :, :, :33] = in_use[..., None]
    written = torch.cat([head, refs, rows.flatten(2)], dim=2)
    assert bool((ref[~written] == FILL).all()) and bool((ref[:, :, :OFF_REF] != FILL).all())
    got = _build(eng, LEAN, c, c_offset)
    diff = got != ref
    if bool(diff.any()):
      where = torch.nonzero(diff)[:8].tolist()
      pytest.fail(f"{kind}, L={L}, {n_cond} conditions: {int(diff.sum())} words differ, first at "
                  f"(condition, layer, word) {where}; pieces {pieces.flatten()[:8].tolist()}")


def test_builder_selection_and_identical_samples(dev):
  """Knob 0: build_tables() picks by table count as documented; knob 1 and 2 give the same sample_logprob bits."""
  eng = _engine(2, _params("random", 2), dev)
  eng.set_pwl_builder(0)
  for n_cond in (1, 16, 48, 1023, 1024, 2048):
    eng.build_tables(torch.linspace(0.0, 1.0, n_cond, device=dev))
    assert eng.last_pwl_builder() == (LEAN if n_cond * 2 >= LEAN_MIN_TABLES else REFERENCE), n_cond
  S, Bs = 7, 9998
  g = torch.Generator(device="cpu").manual_seed(3)
  noise = torch.randn(S * Bs, 2, generator=g).to(dev)
  ts = torch.linspace(0.0, 1.0, S, device=dev)
  eng.set_pwl(2)
  res = {}
  for mode in (REFERENCE, LEAN, 0):
    eng.set_pwl_builder(mode)
    y, lp = eng.sample_logprob(noise, ts)
    assert eng.last_path() == "tables"
    assert eng.last_pwl_builder() == (mode or (LEAN if S * 2 >= LEAN_MIN_TABLES else REFERENCE))
    res[mode] = (y.clone(), lp.clone())
  for mode in (LEAN, 0):
    assert torch.equal(res[mode][0], res[REFERENCE][0]) and torch.equal(res[mode][1], res[REFERENCE][1])
