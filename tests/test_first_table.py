"""The `first` spline's inverse table, construction and certification, on the numpy float64 restatement
(cnf_ot_amd/first_table.py; the device builder is held to it in test_gpu_first_table.py).  CPU only.

1. Every one of the 30 N(0, 0.2^2) parameter sets (seeds 0-29; bench.py's scale) is certified: the cap on uncertified
   sets is zero.
2. A certified table meets the builder's budget -- |d out| <= 2.4e-7 max(1, |out|), the same for ld: two fp32 ulps at
   the value's magnitude -- at a probe set ten times denser than the builder's (170 interior points per piece, none of
   them a node or a builder probe).
3. Ill-conditioned sets are refused: adjacent knot slopes 1e-4 and 40.5, and a bin at the minimum width (two knots in
   one cell).
4. Neighbouring pieces agree at their common edge to 1 fp32 ulp.  Both interpolate the closed form there; what is
   left is the rounding of their coefficients to fp32, half an ulp of its own c0 on either side.  So the ulp is that of
   the larger of the two c0 (they can lie on either side of a power of two), and not below the budget's scale,
   max(1, |value|): ld crosses zero, where an ulp of the value itself means nothing.
5. The lookup as the kernel does it (cell, breakpoint comparison, Horner about ref) reproduces the closed form over the
   whole range within the budget plus the half-ulp rounding of c0.
"""
import functools

import numpy as np
import pytest

from cnf_ot_amd import first_table as ft

SEEDS = tuple(range(30))
DENSE = (2.0 * np.arange(10 * ft.FT_PROBES) + 1.0) / (10 * ft.FT_PROBES) - 1.0


def first_params(seed, scale=0.2):
  """The `first` entries of Params.random(FlowConfig(dim=2), scale, seed): the head of the same PCG64 stream."""
  from cnf_ot_amd import FlowConfig
  n = FlowConfig(dim=2).param_count()
  return np.random.default_rng(seed).normal(0.0, scale, n).astype(np.float32)[:16]


def refused_params(kind):
  p = first_params(42)
  if kind == "slopes":
    p[12], p[13] = -40.0, 40.0       # knot slopes softplus(-40 + o) + 1e-4 and softplus(40 + o) + 1e-4, side by side
  else:
    p[7] = -60.0                     # a height logit 60 below the rest: the bin keeps only min_bin_size
  return p


@functools.lru_cache(maxsize=None)
def table(seed):
  return ft.build(first_params(seed))


def test_every_bench_scale_set_is_certified():
  bad = [s for s in SEEDS if not table(s)["certified"]]
  worst = max(table(s)["err"] for s in SEEDS)
  print(f"\n[first table] 30 sets at scale 0.2: {len(SEEDS) - len(bad)} certified, worst error {worst / ft.FT_BUDGET:.3f} of the budget")
  assert bad == []


@pytest.mark.parametrize("seed", SEEDS)
def test_certified_tables_meet_the_budget_at_dense_probes(seed):
  assert not set(np.round(DENSE, 12)) & set(np.round(np.concatenate([ft._PROBES, ft._NODES]), 12))
  t = ft.build(first_params(seed), probes=DENSE)
  print(f"\n[first table] seed {seed}: {t['err'] / ft.FT_BUDGET:.3f} of the budget at {DENSE.size} probes per piece")
  assert t["geom_ok"] and t["err"] <= ft.FT_BUDGET


@pytest.mark.parametrize("kind", ["slopes", "min_bin"])
def test_ill_conditioned_sets_are_refused(kind):
  t = ft.build(refused_params(kind))
  h = t["header"]
  if kind == "slopes":
    assert h["d"][2] < 1.01e-4 and h["d"][3] > 40.0 and t["geom_ok"]
  else:
    assert h["yk"][3] - h["yk"][2] < 1.001e-4 and not t["geom_ok"]
  assert not t["certified"]


@pytest.mark.parametrize("seed", SEEDS + (42,))
def test_neighbouring_pieces_agree_at_their_edges(seed):
  t = ft.build(first_params(seed))
  assert t["certified"]
  rows, geom = t["rows"].astype(np.float64), t["geom"]
  a, b, ref = (np.array([g[i] for g in geom]) for i in range(3))
  assert np.array_equal(b[:-1], a[1:])
  worst = 0.0
  for col in (0, 1):
    left = ft._horner(rows[:-1, col::2], (b[:-1] - ref[:-1])[:, None])[:, 0]
    right = ft._horner(rows[1:, col::2], (a[1:] - ref[1:])[:, None])[:, 0]
    mag = np.maximum(np.maximum(np.abs(rows[:-1, col]), np.abs(rows[1:, col])), 1.0)
    worst = max(worst, float((np.abs(left - right) / np.spacing(mag.astype(np.float32))).max()))
  print(f"\n[first table] seed {seed}: neighbours differ by at most {worst:.3f} ulp at an edge")
  assert worst <= 1.0


def test_lookup_reproduces_the_closed_form():
  t = table(3)
  h = t["header"]
  v = np.random.default_rng(5).uniform(h["lo"], h["hi"], 200000)
  o, l = ft.evaluate(t, v)
  k = np.clip(np.searchsorted(h["yk"], v, side="right") - 1, 0, h["K"] - 1)
  ro, rl = ft.inverse_closed(h, k, v)
  eo = (np.abs(o - ro) / np.maximum(1.0, np.abs(ro))).max()
  el = (np.abs(l - rl) / np.maximum(1.0, np.abs(rl))).max()
  print(f"\n[first table] lookup over the range: out {eo:.2e}, ld {el:.2e} (budget {ft.FT_BUDGET:.1e})")
  assert eo <= ft.FT_BUDGET and el <= ft.FT_BUDGET
