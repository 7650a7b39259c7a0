"""Host side of the exact score (cnf_score), without a GPU: the symbol is bound, declared and exported; the exact=
flags of utils.score_field / utils.eulerian_fields choose the route they say and their defaults the old one, checked on
a stand-in engine over the float64 restatement tests/flow_fields_f64.py; print_path_errors shows the score column only
where evaluate_path made one."""
import os
import re

import numpy as np
import pytest
import torch

import flow_fields_f64 as ff
import oracle
from cnf_ot_amd import _capi, utils

REPO = os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "..")
T_ARRAY = np.array([0.0, 0.5, 2.0])


def test_cnf_score_is_bound_declared_and_exported():
  assert "cnf_score" in _capi.SYMBOLS
  res, args = _capi.SYMBOLS["cnf_score"]
  assert len(args) == 9          # m, pts, pts_shared, c, n_slices, count, score, log_prob, stream
  header = open(os.path.join(REPO, "include", "cnf_ot_amd.h")).read()
  assert re.search(r"\bint\s+cnf_score\s*\(\s*CnfModel\s*\*m,\s*const float \*pts,\s*int32_t pts_shared", header)
  assert hasattr(_capi.lib(), "cnf_score"), f"cnf_score: not exported by {_capi.LIB_PATH}"
  assert _capi.PATH_NAMES[11] == "score"


class _StandInEngine:
  """What utils asks of FlowEngine for the score, answered by the float64 oracle flow; every call is recorded."""

  def __init__(self, flow):
    self.flow, self.device, self.calls = flow, torch.device("cpu"), []

  def _points(self, t, what, keep_f64=False):
    return t

  def eulerian_fields(self, t, pts=None, grid=None, **kw):
    self.calls.append(("eulerian_fields", {k: v for k, v in kw.items() if v is not None and v is not False}))
    assert grid is None
    res = {}
    if kw.get("score"):
      res["score"] = torch.from_numpy(ff.score_field(self.flow, pts.numpy(), t, kw["dx"]))
    if kw.get("vel"):
      res["vel"] = torch.from_numpy(ff.velocity_field(self.flow, pts.numpy(), t, kw["dt"]))
    return res

  def score(self, pts, cond, shared=False, with_log_prob=False):
    self.calls.append(("score", {"shared": shared}))
    assert pts.dtype == torch.float32
    s = ff.score_field(self.flow, pts.double().numpy(), np.asarray(cond, dtype=np.float64), 2e-6)      # (the derivative's stand-in)
    return torch.from_numpy(s.reshape(-1, pts.shape[1]).astype(np.float32))


class _StandInModel:
  def __init__(self, D, be):
    self.cfg, self._be = type("Cfg", (), {"dim": D})(), be

  def terms_backend(self, params, device=None):
    return self._be


@pytest.fixture()
def stand_in(oracle_lib):
  D = 3
  ocfg = oracle.OracleConfig(D=D)
  params = np.random.default_rng(3).normal(0.0, 0.2, oracle.param_count(ocfg)).astype(np.float32)
  be = _StandInEngine(ff.OracleFlow(ocfg, params))
  pts = torch.from_numpy(np.random.default_rng(2).uniform(-3, 3, (40, D)))
  return _StandInModel(D, be), be, pts


def test_the_defaults_take_the_difference_route(stand_in):
  model, be, pts = stand_in
  want = ff.score_field(be.flow, pts.numpy(), T_ARRAY, 0.02)
  for got in (utils.score_field(model, None, pts, T_ARRAY, dx=0.02),
              utils.score_field(model, None, pts, T_ARRAY, dx=0.02, exact=False),
              utils.eulerian_fields(model, None, pts, T_ARRAY, score=True, dx=0.02)["score"],
              utils.eulerian_fields(model, None, pts, T_ARRAY, score=True, dx=0.02, exact_score=False)["score"]):
    assert np.array_equal(got.numpy(), want)
  assert [c[0] for c in be.calls] == ["eulerian_fields"] * 4          # never the exact entry point
  assert all(c[1]["score"] is True and c[1]["dx"] == 0.02 for c in be.calls)
  # the flag without a score request changes nothing either
  be.calls.clear()
  utils.eulerian_fields(model, None, pts, T_ARRAY, vel=True, exact_score=True)
  assert [c[0] for c in be.calls] == ["eulerian_fields"]


def test_exact_takes_the_score_from_the_exact_entry_point(stand_in):
  model, be, pts = stand_in
  p32 = pts.to(torch.float32)
  s = utils.score_field(model, None, p32, T_ARRAY, dx=123.0, exact=True)          # dx is ignored
  assert s.shape == (3, 40, 3) and s.dtype == torch.float32
  assert be.calls == [("score", {"shared": True})]
  be.calls.clear()
  res = utils.eulerian_fields(model, None, p32, T_ARRAY, vel=True, score=True, exact_score=True, dt=0.02)
  assert sorted(res) == ["score", "vel"] and torch.equal(res["score"], s)
  # the other fields from the fused launch as before: asked without the score
  assert be.calls == [("score", {"shared": True}), ("eulerian_fields", {"vel": True, "dt": 0.02, "dtype": torch.float32})]
  assert np.array_equal(res["vel"].numpy(), ff.velocity_field(be.flow, p32.double().numpy(), T_ARRAY, 0.02))


def test_exact_refuses_float64_before_any_work(stand_in):
  model, be, pts = stand_in
  for kw in (dict(), dict(dtype=torch.float64)):          # float64 points, or float64 asked for
    with pytest.raises(_capi.CnfError) as ei:
      utils.score_field(model, None, pts if not kw else pts.to(torch.float32), T_ARRAY, exact=True, **kw)
    assert ei.value.code == _capi.CNF_ERR_UNSUPPORTED
  with pytest.raises(_capi.CnfError):
    utils.eulerian_fields(model, None, pts, T_ARRAY, vel=True, score=True, exact_score=True)
  assert be.calls == []
  # ... and float64 points cast down on request are served
  assert utils.score_field(model, None, pts, T_ARRAY, dtype=torch.float32, exact=True).shape == (3, 40, 3)


def test_path_table_prints_the_score_column_only_when_it_is_there(capsys):
  from cnf_ot_amd import solvers
  res = {"times": [0.0, 1.0], "density_sq_err": [1e-3, 2e-3], "velocity_rel_err": [0.5, 0.25], "action_exact": [1.0, 2.0],
         "mass": [0.99, 0.98]}
  solvers.print_path_errors(res)
  plain = capsys.readouterr().out
  assert "score" not in plain and plain.count("\n") == 3
  assert "  1.0000 | 2.000e-03 | 2.500e-01 | 2.000000 | 0.980000\n" in plain
  solvers.print_path_errors(dict(res, score_rel_err=[0.125, 0.0625]))
  with_score = capsys.readouterr().out
  assert with_score.splitlines()[0].endswith("| score rel err")
  assert with_score.splitlines()[2] == "  1.0000 | 2.000e-03 | 2.500e-01 | 2.000000 | 0.980000 | 6.250e-02"
