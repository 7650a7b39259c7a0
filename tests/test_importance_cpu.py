"""Host side of the importance-sampling diagnostics, without a GPU: the float64 helper against closed forms on the
identity flow, the underflow the reference's linear-space arithmetic runs into, merge_importance_stats, the target
packer, the workspace query and the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import importance_ref as ir
import oracle
from cnf_ot_amd import _capi, applications, solvers

REPO = os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "..")


def _identity_flow(oracle_lib, D, n, seed):
  """(samples, log_prob) of the identity flow (all parameters zero) on n draws of the build's Philox stream"""
  ocfg = oracle.OracleConfig(D=D)
  noise = oracle.normal(seed, 0, n * D).reshape(n, D)
  y, lq = oracle.sample_logprob(ocfg, np.zeros(oracle.param_count(ocfg)), noise, [0.5])
  assert np.abs(y - noise).max() <= 1e-12          # the identity
  return y, lq


@pytest.mark.parametrize("D,s,ess_frac,kl", [(2, 0.7, 0.91, 0.0719), (10, 1.2, 0.8154, 0.0783)])
def test_closed_forms_on_the_identity_flow(oracle_lib, D, s, ess_frac, kl):
  """q = N(0, I), p = N(0, s I): KL = D/2 (1/s - 1 + log s), ESS/n = (2 s - s^2)^(D/2), log Z = 0"""
  assert abs(0.5 * D * (1.0 / s - 1.0 + np.log(s)) - kl) < 5e-5 and abs((2 * s - s * s) ** (0.5 * D) - ess_frac) < 5e-5
  n = 65536
  y, lq = _identity_flow(oracle_lib, D, n, seed=7)
  tg = applications.GaussianMixtureTarget(np.zeros((1, D)), s)
  got = ir.summary(ir.log_weights(tg, y, lq))
  print(f"D={D} s={s}: log_Z={got['log_Z']:+.5f} KL={got['KL']:.5f} (exact {kl}) ess/n={got['ess'] / n:.5f} (exact {ess_frac})")
  assert abs(got["log_Z"]) <= 0.01
  assert abs(got["KL"] - 0.5 * D * (1.0 / s - 1.0 + np.log(s))) <= 0.01
  assert abs(got["ess"] / n - (2 * s - s * s) ** (0.5 * D)) <= 0.02
  # ... and the same numbers from the raw, mergeable state
  raw = ir.summary_of_raw(ir.raw_state(ir.log_weights(tg, y, lq)))
  for k in ("log_Z", "KL", "ess"):
    assert abs(raw[k] - got[k]) <= 1e-12 * max(1.0, abs(got[k]))


def test_the_linear_space_formula_underflows_where_the_log_space_one_does_not(oracle_lib):
  n = 4096
  y, lq = _identity_flow(oracle_lib, 2, n, seed=3)
  tg = applications.GaussianMixtureTarget([[40.0, 40.0]])
  lw = ir.log_weights(tg, y, lq)
  nv = ir.naive(lw + lq, lq)
  assert nv["Z"] == 0.0 and not np.isfinite(nv["ess"])          # sum w underflows: Z = 0, ESS = 0 / 0
  got = ir.summary(lw)
  assert np.isfinite(got["log_Z"]) and -1700.0 < got["log_Z"] < -1000.0
  assert 1.0 <= got["ess"] <= n and got["ess"] < 10.0          # a handful of samples carry all the weight
  # the torch summary of the raw state agrees
  s = applications.importance_summary(torch.from_numpy(ir.raw_state(lw)[None]))
  assert abs(float(s["log_Z"][0]) - got["log_Z"]) <= 1e-12 * abs(got["log_Z"])
  assert abs(float(s["ess"][0]) - got["ess"]) <= 1e-12 * got["ess"]


@pytest.mark.parametrize("cuts", [[], [700], [1, 1], [5, 5, 100, 101, 1000, 1001, 3999]])
def test_merge_reproduces_the_whole(cuts):
  """1, 2, 3 and 8 uneven parts, one of them empty (a repeated cut)"""
  rng = np.random.default_rng(5)
  S, n = 3, 4000
  lw = rng.normal(0.0, 1.0, (S, n)) * np.array([[1.0], [30.0], [300.0]]) - np.array([[0.0], [50.0], [900.0]])
  whole = np.stack([ir.raw_state(lw[s]) for s in range(S)])
  edges = [0] + list(cuts) + [n]
  parts = [torch.from_numpy(np.stack([ir.raw_state(lw[s, a:b]) for s in range(S)])) for a, b in zip(edges[:-1], edges[1:])]
  assert len(parts) == len(cuts) + 1 and any(float(p[0, 4]) == 0.0 for p in parts) == (len(cuts) in (2, 7))
  got = applications.merge_importance_stats(parts).numpy()
  assert got.shape == (S, 5) and np.array_equal(got[:, 0], whole[:, 0]) and np.array_equal(got[:, 4], whole[:, 4])
  assert np.abs(got / whole - 1.0).max() <= 1e-12
  # NaN (a slice with a non-finite log-weight) stays NaN, the other slices are untouched
  bad = parts[0].clone()
  bad[1, :4] = float("nan")
  got_bad = applications.merge_importance_stats([bad] + parts[1:]).numpy()
  assert np.isnan(got_bad[1, :4]).all() and got_bad[1, 4] == n and np.array_equal(got_bad[[0, 2]], got[[0, 2]])


def test_the_packer():
  A = np.array([[5.0, 1.0], [1.0, 0.5]])
  tg = applications.GaussianMixtureTarget([[-3.0, -3.0]], A)
  assert np.abs(tg.W.T @ tg.W @ A - np.eye(2)).max() <= 1e-12 and tg.W[0, 1] == 0.0
  assert abs(tg.log_det_W + 0.5 * np.log(np.linalg.det(A))) <= 1e-12
  s = tg.spec
  assert s.n_comp == 1 and [s.W[0][0], s.W[1][0], s.W[1][1]] == [tg.W[0, 0], tg.W[1, 0], tg.W[1, 1]] and s.W[0][1] == 0.0
  assert s.mean[0][0] == -3.0 and s.log_weight[0] == 0.0 and s.log_weight[1] == -np.inf and s.scale is None
  mix = applications.GaussianMixtureTarget(applications.MIXTURE_CENTERS, weights=[1, 1, 2, 2, 1, 1, 4, 4])
  assert mix.n_comp == 8 and abs(np.exp(mix.log_weights).sum() - 1.0) <= 1e-15 and mix.spec.log_weight[6] == np.log(0.25)
  assert applications.GaussianMixtureTarget(np.zeros(5), 2.0).W[3, 3] == pytest.approx(2.0 ** -0.5, rel=1e-15)
  for bad in (dict(means=np.zeros((1, 2)), cov=np.array([[1.0, 2.0], [2.0, 1.0]])),      # indefinite
              dict(means=np.zeros((1, 2)), cov=0.0),
              dict(means=np.zeros((1, 2)), cov=-1.0),
              dict(means=np.zeros((9, 2))),                                              # more than 8 components
              dict(means=np.zeros((1, 15)))):                                            # dim > 14
    with pytest.raises(ValueError):
      applications.GaussianMixtureTarget(**bad)


def test_known_densities_and_the_fit_table(capsys):
  assert list(applications.FP_FIT_TIMES) == solvers.FIGURE_SETTINGS[("fp", None, 2)]["times"]
  ot = applications.known_densities(solvers.load_config(overrides={"general": {"type": "ot"}}))
  assert [e[0] for e in ot] == [0.0, 1.0] and ot[0][1].n_comp == 8 and ot[1][1].n_comp == 1 and ot[1][2] is None
  og = applications.known_densities(solvers.load_config(overrides={"general": {"type": "ot"}, "ot": {"source": "gaussian"}}))
  assert np.array_equal(og[0][1].cov, [[5.0, 1.0], [1.0, 0.5]]) and np.array_equal(og[0][1].means, [[-3.0, -3.0]])
  rw = applications.known_densities(solvers.load_config())
  assert len(rw) == 1 and rw[0][0] == 0.0 and rw[0][1].cov[0, 0] == pytest.approx(0.6)      # 2 (T + 1) / beta
  fp = applications.known_densities(solvers.load_config(overrides={"general": {"type": "fp", "dim": 10}}))
  assert len(fp) == 1 and fp[0][1].dim == 10 and fp[0][1].cov[9, 9] == 1.0                  # (T + 1) / 2
  ou = applications.known_densities(solvers.load_config(overrides={"general": {"type": "fp"},
                                                                   "fp": {"velocity_field_type": "ou"}}))
  assert [e[0] for e in ou] == [0.0, 0.05, 0.1, 0.3, 1.0] and all(e[1] is ou[0][1] for e in ou)
  assert ou[0][2] == 1.0 and ou[-1][2] == pytest.approx(applications.ou_variance(1.0, 1, 1.0, 0.5))
  solvers.print_fit({"batch_size": 8, "times": [0.0, 1.0], "log_Z": [1e-3, -2.0], "KL": [0.5, 0.25], "ess_pct": [99.5, 12.25],
                     "max_log_w": [0.1, 3.0]})
  out = capsys.readouterr().out.splitlines()
  assert len(out) == 3 and out[2] == "  1.0000 | -2.0000e+00 | 2.5000e-01 | 12.25 | 3.000"


def test_workspace_query_and_bindings():
  lib = _capi.lib()
  n = ctypes.c_int64(-1)
  assert lib.cnf_importance_workspace(3, 700, 2, ctypes.byref(n)) == _capi.CNF_OK and n.value > 0
  big = ctypes.c_int64(-1)
  assert lib.cnf_importance_workspace(5, 1 << 20, 10, ctypes.byref(big)) == _capi.CNF_OK and big.value >= n.value
  assert lib.cnf_importance_workspace(0, 0, 2, ctypes.byref(n)) == _capi.CNF_OK and n.value > 0
  for args in ((-1, 700, 2), (3, -1, 2), (3, 700, 15), (3, 700, 0)):
    assert lib.cnf_importance_workspace(*args, ctypes.byref(n)) == _capi.CNF_ERR_INVALID, args
  assert lib.cnf_importance_workspace(3, 700, 2, None) == _capi.CNF_ERR_INVALID
  header = open(os.path.join(REPO, "include", "cnf_ot_amd.h")).read()
  for name in ("cnf_importance_workspace", "cnf_importance_stats", "cnf_importance_stats_seeded"):
    assert name in _capi.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header, name
  assert len(_capi.SYMBOLS["cnf_importance_stats"][1]) == 11 and len(_capi.SYMBOLS["cnf_importance_stats_seeded"][1]) == 12
  assert _capi.PATH_NAMES[12] == "importance"
  assert re.search(r"tests/test_fit_prob\.py:50-56", header)
  # the struct the kernels read: the layout include/cnf_ot_amd.h declares
  assert ctypes.sizeof(_capi.CnfTargetSpec) == 8 + 8 * (8 * 14 + 8 + 14 * 14 + 1) + 8
  assert _capi.CnfTargetSpec.mean.offset == 8 and _capi.CnfTargetSpec.W.offset == 8 + 8 * (8 * 14 + 8)
