"""CPU tests of the interaction energy: the float64 restatement (tests/interaction_ref.py) the GPU tests hold
cnf_interaction to -- pinned against closed forms, and its gradient and force against central differences of its own
value -- the host-side argument checks of cnf_interaction through the C ABI (no device is touched), the Python entry
points' refusals, which come before any device work, and the config section.

Closed forms (N = 4 000, scale 1.2, fixed seeds): the Gaussian pair mean lies within 5 standard errors of
(bw^2 / (bw^2 + 2 s^2))^(D / 2) and, at D = 1, the exponential pair mean within 5 of exp(tau^2 / (2 bw^2)) erfc(tau /
(sqrt 2 bw)), tau^2 = 2 s^2.  The standard error of a pair mean is read from the restatement's own row means r_i: a
U-statistic's variance is 4 var(r) / N to leading order.  The quadratic kind is an identity:
sum_{i != j} |x_i - x_j|^2 / 2 = N sum_i |x_i - mean|^2.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interaction_ref as ir

SIGNED = {"gaussian": ir.spec("gaussian", [1.0, -0.5], [0.8, 1.7]), "exponential": ir.spec("exponential", [1.0, -0.5], [0.5, 2.0]),
          "quadratic": ir.spec("quadratic", [-0.7])}


@pytest.mark.parametrize("D", [1, 2, 10])
def test_restatement_against_the_closed_forms(D):
  N, s = 4000, 1.2
  x = ir.cloud(D, N, seed=100 + D, scale=s)
  cases = [(ir.spec("gaussian", [1.0], [math.sqrt(D)]), ir.population_gaussian(D, s, math.sqrt(D)))]
  if D == 1:
    cases += [(ir.spec("exponential", [1.0], [bw]), ir.population_exponential_1d(s, bw)) for bw in (0.5, 2.0)]
  for sp, pop in cases:
    got = ir.sums(x, sp) / (N * (N - 1.0))
    r = ir.row_means(x, sp)
    assert abs(r.mean() - got) <= 1e-12 and got == 2.0 * ir.energy(x, sp)
    se = 2.0 * r.std(ddof=1) / math.sqrt(N)
    print(f"[interaction closed form D={D}] {sp['kind']} bw {sp['bw'][0]:.3f}: {got:.6f} against {pop:.6f}, "
          f"{abs(got - pop) / se:.2f} standard errors of {se:.2e}")
    assert abs(got - pop) <= 5.0 * se, (sp, got, pop, se)
  # the quadratic identity and its force
  sp = ir.spec("quadratic", [1.0])
  x64 = x.astype(np.float64)
  c = x64 - x64.mean(0)
  lhs, rhs = ir.sums(x, sp), N * (c * c).sum()
  print(f"[interaction closed form D={D}] quadratic identity: relative {abs(lhs - rhs) / rhs:.1e}")
  assert abs(lhs - rhs) <= 1e-12 * rhs
  assert np.abs(ir.force(x, sp) - N / (N - 1.0) * c).max() <= 1e-12 * np.abs(c).max()
  assert abs(ir.energy(x, sp) - 0.5 * np.trace(np.atleast_2d(np.cov(x64.T)))) <= 1e-12 * ir.energy(x, sp)


@pytest.mark.parametrize("kind", ["gaussian", "exponential", "quadratic"])
def test_xgrad_and_query_force_against_central_differences(kind):
  D, N, h = 3, 37, 1e-6
  x = ir.cloud(D, N, seed=7).astype(np.float64)
  q = ir.cloud(D, 5, seed=8).astype(np.float64)
  sp = SIGNED[kind]
  g, f = ir.xgrad(x, sp), ir.force(x, sp, q)
  assert g.shape == (N, D) and f.shape == (5, D)
  worst_g = worst_f = 0.0
  for d in range(D):
    for i in (0, 5, N - 1):
      xp, xm = x.copy(), x.copy()
      xp[i, d] += h
      xm[i, d] -= h
      worst_g = max(worst_g, abs((ir.energy(xp, sp) - ir.energy(xm, sp)) / (2.0 * h) - g[i, d]))
    for i in (0, 4):
      qp, qm = q.copy(), q.copy()
      qp[i, d] += h
      qm[i, d] -= h
      worst_f = max(worst_f, abs((ir.potential(x, sp, qp)[i] - ir.potential(x, sp, qm)[i]) / (2.0 * h) - f[i, d]))
  print(f"[interaction {kind}] central differences: xgrad {worst_g:.2e}, query force {worst_f:.2e}")
  # values are O(1) in float64 (rounding 1e-16 / h = 1e-10) and smooth away from coincident points (h^2 = 1e-12)
  assert worst_g <= 1e-8 and worst_f <= 1e-8
  # self-mode force = N dF / dx; coincident points: finite, and equal points get equal forces
  assert np.abs(ir.force(x, sp) - g * N).max() <= 4e-16 * np.abs(g * N).max()      # (one division's rounding)
  xd = np.concatenate([x, x[:4]])
  fd = ir.force(xd, sp)
  assert np.isfinite(fd).all() and np.allclose(fd[:4], fd[N:N + 4], rtol=0, atol=1e-15)


def _spec(kind=0, amp=(1.0, -0.5), bw=(0.5, 2.0), n_terms=None):
  from cnf_ot_amd import _capi
  s = _capi.CnfInteractionSpec()
  s.kind, s.n_terms = kind, len(amp) if n_terms is None else n_terms
  for i, a in enumerate(amp[:4]):
    s.amp[i] = a
  for i, b in enumerate(bw[:4]):
    s.bw[i] = b
  return s


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  nbytes, small = ctypes.c_int64(0), ctypes.c_int64(0)
  assert lib.cnf_interaction_workspace(3, 300, 0, 10, 1, ctypes.byref(nbytes)) == _capi.CNF_OK
  P = lib.cnf_interaction_splits(3, 300, 0, 10)
  assert P >= 1 and nbytes.value == 8 * 3 * P * 300 * (1 + 10)
  assert lib.cnf_interaction_workspace(3, 300, 0, 10, 0, ctypes.byref(small)) == _capi.CNF_OK and small.value == 8 * 3 * P * 300
  qbytes = ctypes.c_int64(0)
  assert lib.cnf_interaction_workspace(3, 300, 257, 10, 1, ctypes.byref(qbytes)) == _capi.CNF_OK
  assert qbytes.value == 8 * 3 * lib.cnf_interaction_splits(3, 300, 257, 10) * 257 * 11
  # the split count is a function of the sizes alone: 1 while the sources are one tile of 64 columns
  assert lib.cnf_interaction_splits(1, 64, 0, 2) == 1 and lib.cnf_interaction_splits(1, 65, 0, 2) == 2
  assert lib.cnf_interaction_splits(32, 4096, 0, 2) == 8 and lib.cnf_interaction_splits(9, 32768, 0, 10) == 4
  assert lib.cnf_interaction_splits(1, 64, 1 << 20, 2) == 1
  for bad in ((0, 300, 0, 10), (65, 300, 0, 10), (3, 1, 0, 10), (3, 300, -1, 10), (3, 300, 0, 0), (3, 300, 0, 15),
              (3, (1 << 20) + 1, 0, 2), (3, 300, (1 << 20) + 1, 2)):
    assert lib.cnf_interaction_workspace(*bad, 1, ctypes.byref(small)) == _capi.CNF_ERR_INVALID, bad
    assert lib.cnf_interaction_splits(*bad) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_interaction_workspace(3, 300, 0, 10, 1, None) == _capi.CNF_ERR_INVALID
  assert lib.cnf_interaction_workspace(3, 300, 0, 10, 0, ctypes.byref(small)) == _capi.CNF_OK

  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  good = dict(spec=_spec(), S=3, x=4096, N=300, q=None, Q=0, D=10, sums=12288, pot=16384, force=20480, ws=24576,
              wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_interaction(None if a["spec"] is None else ctypes.byref(a["spec"]), a["S"], a["x"], a["N"], a["q"],
                               a["Q"], a["D"], a["sums"], a["pot"], a["force"], a["ws"], a["wsb"], None)

  inf, nan = float("inf"), float("nan")
  for bad in ({"spec": None}, {"x": None}, {"sums": None}, {"ws": None}, {"D": 0}, {"D": 15}, {"N": 1}, {"N": (1 << 20) + 1},
              {"S": 0}, {"S": 65}, {"q": 8192}, {"Q": 5}, {"q": 8192, "Q": -1}, {"q": 8192, "Q": (1 << 20) + 1},
              {"spec": _spec(kind=3)}, {"spec": _spec(kind=-1)}, {"spec": _spec(n_terms=0)}, {"spec": _spec(n_terms=5)},
              {"spec": _spec(amp=(1.0, 0.0))}, {"spec": _spec(amp=(1.0, inf))}, {"spec": _spec(amp=(nan, 1.0))},
              {"spec": _spec(bw=(1.0, 0.0))}, {"spec": _spec(bw=(1.0, -2.0))}, {"spec": _spec(bw=(inf, 1.0))},
              {"spec": _spec(bw=(nan, 1.0))}, {"spec": _spec(bw=(1e-30, 1.0))}, {"spec": _spec(kind=1, bw=(1e-30, 1.0))},
              {"spec": _spec(amp=(1e30, 1.0), bw=(1e-6, 1.0))}, {"spec": _spec(kind=2, amp=(0.0,))},
              {"spec": _spec(kind=2, amp=(nan,))}, {"wsb": nbytes.value - 8}, {"force": None, "wsb": small.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad


class _NoEngine:
  """A model whose terms backend is not the HIP engine"""
  def terms_backend(self, params, device=None):
    import torch
    return type("Backend", (), {"device": torch.device("cpu")})()


def test_python_entry_points_refuse_before_the_device():
  import torch
  from cnf_ot_amd import applications as app, autograd, solvers, utils
  from cnf_ot_amd.distributed import Shard
  from cnf_ot_amd.flows import DeviceRng
  x = np.zeros((5, 3), dtype=np.float32)
  inf, nan = float("inf"), float("nan")
  bad_specs = ({"kind": "coulomb"}, {"amplitudes": [1.0] * 5, "bandwidths": [1.0] * 5}, {"amplitudes": [], "bandwidths": []},
               {"amplitudes": [1.0, 2.0], "bandwidths": [1.0]}, {"amplitudes": [0.0]}, {"amplitudes": [inf]},
               {"amplitudes": [nan]}, {"bandwidths": [0.0]}, {"bandwidths": [-1.0]}, {"bandwidths": [inf]},
               {"bandwidths": [nan]}, {"bandwidths": [1e-30]}, {"amplitudes": [1e30], "bandwidths": [1e-6]},
               {"kind": "exponential", "bandwidths": [1e-30]}, {"kind": "quadratic", "amplitudes": [0.0]},
               {"kind": "quadratic", "amplitudes": [1.0, 2.0]}, {"kind": "quadratic", "amplitudes": [nan]})
  for bad in bad_specs:
    kw = dict(dict(kind="gaussian", amplitudes=[1.0], bandwidths=[1.0]), **bad)
    for call in (lambda: utils.interaction_spec(**kw), lambda: utils.interaction_energy(x, **kw),
                 lambda: utils.interaction_field(x, x, **kw), lambda: autograd.interaction_energy(torch.zeros(5, 3), **kw),
                 lambda: app.interaction_loss_fn(None, 3, None, [0.5], 0, 96, shard=Shard(0, 1), **kw)):
      with pytest.raises(ValueError):
        call()
  s = utils.interaction_spec("exponential", [1.0, -0.5], [0.5, 2.0])
  assert (s.kind, s.n_terms, list(s.amp)[:2], list(s.bw)[:2]) == (1, 2, [1.0, -0.5], [0.5, 2.0])
  assert utils.interaction_spec("quadratic").amp[0] == 1.0 and utils.interaction_spec("gaussian").n_terms == 1
  for shape in ((1, 1, 3), (0, 5, 3), (65, 5, 3), (1, 5, 0), (1, 5, 15), (1, (1 << 20) + 1, 2)):
    with pytest.raises(ValueError):
      utils.interaction_check_shapes(shape)
  utils.interaction_check_shapes((2, 5, 3), (2, 1, 3))
  for qs in ((3, 7, 3), (2, 7, 2), (2, 0, 3), (2, (1 << 20) + 1, 3), (2, 7)):
    with pytest.raises(ValueError):
      utils.interaction_check_shapes((2, 5, 3), qs)
  for bad in (x[:1], np.zeros(5), np.zeros((65, 5, 3)), np.zeros((5, 15))):
    with pytest.raises(ValueError):
      utils.interaction_energy(bad, "quadratic")
  with pytest.raises(ValueError):
    utils.interaction_field(np.zeros((7, 2)), x, "quadratic")
  with pytest.raises(ValueError):
    utils.interaction_field(np.zeros((2, 7, 3)), x, "quadratic")
  # the training term: world > 1, B < 2, a backend that is not the HIP engine
  with pytest.raises(ValueError, match="all-gather"):
    app.interaction_loss_fn(None, 2, None, [0.5], 0, 96, "quadratic", shard=Shard(0, 2))
  with pytest.raises(ValueError):
    app.interaction_loss_fn(None, 2, None, [0.5], 0, 1, "quadratic", shard=Shard(0, 1))
  with pytest.raises(ValueError, match="HIP engine"):
    app.interaction_loss_fn(_NoEngine(), 2, None, [0.5], 0, 96, "quadratic", shard=Shard(0, 1))
  # the composites: a captured step's rng, world > 1, sub < 2, a bad spec -- each before the backend is asked for
  given = ({"kind": "quadratic"}, 0.5)
  rng_dev = DeviceRng.__new__(DeviceRng)      # (no device behind it: only its type is read)
  for name, fn in (("ot", lambda **kw: app.ot_loss_fn(None, 2, 1, 0.01, 4, "free", None, kw.pop("rng", 0), 5000.0,
                                                      kw.pop("batch_size", 2048), **kw)),
                   ("rwpo", lambda **kw: app.rwpo_loss_fn(None, 2, 2, 10, 0.01, 0.01, 4, "double_well", 1, None,
                                                          kw.pop("rng", 0), 5000.0, kw.pop("batch_size", 2048), **kw))):
    with pytest.raises(ValueError, match="eager update only"):
      fn(rng=rng_dev, interaction=given, shard=Shard(0, 1))
    with pytest.raises(ValueError, match="all-gather"):
      fn(interaction=given, shard=Shard(0, 2))
    with pytest.raises(ValueError, match="batch_size // 32"):
      fn(batch_size=63, interaction=given, shard=Shard(0, 1))
    with pytest.raises(ValueError):
      fn(interaction=({"kind": "gaussian", "bandwidths": [-1.0]}, 1.0), shard=Shard(0, 1))
  # the solver: fp has no interaction term; a captured run is refused before the model is built; the evaluation
  ia = {"interaction": {"kind": "gaussian", "strength": 2.0, "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}}
  with pytest.raises(ValueError, match="fp_loss_fn"):
    solvers.bind_loss(solvers.load_config(overrides=dict(ia, general={"type": "fp"})), None)
  for _type in ("ot", "rwpo"):
    fn = solvers.bind_loss(solvers.load_config(overrides=dict(ia, general={"type": _type})), None)
    kw, strength = fn.keywords["interaction"]
    assert strength == 2.0 and kw == {"kind": "gaussian", "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}
    assert "interaction" not in solvers.bind_loss(solvers.load_config(overrides={"general": {"type": _type}}), None).keywords
  with pytest.raises(ValueError, match="eager update only"):
    solvers.train(solvers.load_config(overrides=ia), epochs=1, capture=True)
  with pytest.raises(ValueError):
    solvers.evaluate_interaction(solvers.load_config(), None, None)      # kind "none"
  for kw in ({"n": 2}, {"times": np.linspace(0, 1, 3), "n": (1 << 21) + 2}):
    with pytest.raises(ValueError):
      solvers.evaluate_interaction(solvers.load_config(overrides=ia), None, None, **kw)
  with pytest.raises(ValueError):
    solvers.evaluate_interaction(solvers.load_config(overrides={"interaction": {"kind": "gaussian", "bandwidths": [0.0]}}),
                                 None, None)
  assert solvers._parse(["--interaction"]).interaction and not solvers._parse([]).interaction
  with pytest.raises(ValueError):      # (the checked-in default has kind "none": refused before any training step)
    solvers.main(solvers.load_config(), interaction=True)


def test_load_config_carries_the_section_and_leaves_the_rest(tmp_path):
  from cnf_ot_amd import solvers
  before = {
    "general": {"type": "rwpo", "dim": 2, "dx": 0.01, "dt": 0.01, "t_batch_size": 1, "seed": 42},
    "ot": {"subtype": "free"},
    "rwpo": {"T": 2, "beta": 10, "a": 1, "pot_type": "double_well"},
    "fp": {"T": 1, "a": 1, "sigma": 0.5, "velocity_field_type": "gradient"},
    "cnf": {"flow_num_layers": 2, "mlp_num_layers": 2, "hidden_size": 16, "num_bins": 5},
    "train": {"epochs": 30000, "lr": 0.001, "_lambda": 5000.0, "batch_size": 2048, "eval_frequency": 100},
  }
  cfg = solvers.load_config()
  assert cfg.pop("interaction") == {"kind": "none", "strength": 1.0, "amplitudes": [1.0], "bandwidths": [1.0]}
  assert cfg == before
  # a yaml file's section is merged; sections the loader does not know stay out
  import yaml      # (what load_config itself reads a file with)
  path = tmp_path / "mfc.yaml"
  path.write_text(yaml.safe_dump({"interaction": {"kind": "exponential", "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]},
                                  "hydra": {"run": {"dir": "."}}, "general": {"dim": 3}}))
  cfg = solvers.load_config(str(path))
  assert cfg["interaction"] == {"kind": "exponential", "strength": 1.0, "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}
  assert "hydra" not in cfg and cfg["general"]["dim"] == 3 and cfg["train"] == before["train"]
  assert solvers.load_config()["interaction"]["kind"] == "none"      # (the defaults were not written to)
