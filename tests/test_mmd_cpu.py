"""CPU tests of the kernel two-sample statistics: the float64 restatement (tests/mmd_ref.py) the GPU tests hold cnf_mmd2
to -- pinned against the closed form of a Gaussian kernel's mean between two Gaussians, and its gradient against central
differences of its own value -- the host-side argument checks of cnf_mmd2 through the C ABI (no device is touched), and
the Python entry points' refusals, which come before any device work.

Closed form (N = M = 4 000, fixed seeds): each of the three pair means lies within 5 standard errors of
(bw^2 / (bw^2 + s1^2 + s2^2))^(D / 2) exp(-|mu|^2 / (2 (bw^2 + s1^2 + s2^2))).  The standard error of a pair mean is read
from the restatement's own row (and column) means r_i: a U-statistic's variance is 4 var(r) / N to leading order, the
two-sample mean's var(r) / N + var(c) / M.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_ref as mr


@pytest.mark.parametrize("D", [1, 2, 10])
def test_restatement_against_the_closed_form(D):
  N = M = 4000
  shift, s2 = 0.5, 1.2
  x, y = mr.clouds(D, N, M, seed=100 + D, shift=shift, scale=s2)
  bw = math.sqrt(D)
  sp = mr.spec("gaussian", [bw])
  s = mr.sums(x, y, sp)
  got = (s[0] / (N * (N - 1.0)), s[1] / (M * (M - 1.0)), s[2] / (float(N) * M))
  pop = (mr.population_gaussian(D, 0.0, 1.0, 1.0, bw), mr.population_gaussian(D, 0.0, s2, s2, bw),
         mr.population_gaussian(D, shift * math.sqrt(D), 1.0, s2, bw))
  rxx, ryy = mr.row_means(x, x, sp, True), mr.row_means(y, y, sp, True)
  rxy, cxy = mr.row_means(x, y, sp, False), mr.row_means(y, x, sp, False)
  # the row means reproduce the sums they are the standard error of
  assert abs(rxx.mean() - got[0]) <= 1e-12 and abs(rxy.mean() - got[2]) <= 1e-12 and abs(cxy.mean() - got[2]) <= 1e-12
  se = (2.0 * rxx.std(ddof=1) / math.sqrt(N), 2.0 * ryy.std(ddof=1) / math.sqrt(M),
        math.sqrt(rxy.var(ddof=1) / N + cxy.var(ddof=1) / M))
  for name, g, p, e in zip(("xx", "yy", "xy"), got, pop, se):
    print(f"[mmd closed form D={D}] {name}: {g:.6f} against {p:.6f}, {abs(g - p) / e:.2f} standard errors of {e:.2e}")
    assert abs(g - p) <= 5.0 * e, (name, g, p, e)
  m2 = mr.mmd2_of_sums(s, N, M)
  assert abs(m2 - mr.population_mmd2(D, shift * math.sqrt(D), 1.0, s2, [bw])) <= 5.0 * (se[0] + se[1] + 2.0 * se[2])
  assert m2 == mr.mmd2(x, y, sp)


@pytest.mark.parametrize("kind", ["gaussian", "energy"])
def test_xgrad_against_central_differences(kind):
  D, N, M = 3, 37, 29
  x, y = mr.clouds(D, N, M, seed=7)
  x, y = x.astype(np.float64), y.astype(np.float64)
  sp = mr.spec(kind, [0.8, 1.7, 3.0] if kind == "gaussian" else ())
  g = mr.xgrad(x, y, sp)
  assert g.shape == (N, D)
  h = 1e-6
  worst = 0.0
  for i in (0, 5, N - 1):
    for d in range(D):
      xp, xm = x.copy(), x.copy()
      xp[i, d] += h
      xm[i, d] -= h
      fd = (mr.mmd2(xp, y, sp) - mr.mmd2(xm, y, sp)) / (2.0 * h)
      worst = max(worst, abs(fd - g[i, d]))
  print(f"[mmd xgrad {kind}] central differences: {worst:.2e}")
  # the value is O(1) in float64 (rounding 1e-16 / h = 1e-10) and smooth away from coincident points (h^2 = 1e-12)
  assert worst <= 1e-8
  # coincident points: the energy gradient's term is 0, the Gaussian's vanishes with the difference
  xd = np.concatenate([x, x[:4]])
  yd = np.concatenate([y, x[:3]])
  gd = mr.xgrad(xd, yd, sp)
  assert np.isfinite(gd).all() and np.array_equal(gd[:4], gd[N:N + 4])


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_mmd_workspace(3, 300, 257, 10, 1, ctypes.byref(nbytes)) == _capi.CNF_OK
  P = lib.cnf_mmd_splits(3, 300, 257, 10)
  assert P >= 1 and nbytes.value == 8 * 3 * P * (2 * 300 + 257 + 2 * 300 * 10)
  small = ctypes.c_int64(0)
  assert lib.cnf_mmd_workspace(3, 300, 257, 10, 0, ctypes.byref(small)) == _capi.CNF_OK and small.value < nbytes.value
  # the split count is a function of the sizes alone: 1 while the longer side is one tile of 64 columns
  assert lib.cnf_mmd_splits(1, 64, 64, 2) == 1 and lib.cnf_mmd_splits(1, 65, 64, 2) == 2
  assert lib.cnf_mmd_splits(8, 2048, 2048, 2) == 16 and lib.cnf_mmd_splits(9, 32768, 32768, 10) == 2
  for bad in ((0, 300, 257, 10), (65, 300, 257, 10), (3, 1, 257, 10), (3, 300, 1, 10), (3, 300, 257, 0),
              (3, 300, 257, 15), (3, (1 << 24) + 1, 257, 2)):
    assert lib.cnf_mmd_workspace(*bad, 1, ctypes.byref(small)) == _capi.CNF_ERR_INVALID, bad
    assert lib.cnf_mmd_splits(*bad) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_mmd_workspace(3, 300, 257, 10, 1, None) == _capi.CNF_ERR_INVALID

  def spec(kind=0, bws=(1.0, 2.0)):
    s = _capi.CnfMmdSpec()
    s.kind, s.n_bw = kind, len(bws)
    for i, b in enumerate(bws[:8]):
      s.bw[i] = b
    return s

  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  good = dict(spec=spec(), S=3, x=4096, N=300, y=8192, M=257, D=10, sums=12288, xgrad=16384, ws=20480, wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_mmd2(None if a["spec"] is None else ctypes.byref(a["spec"]), a["S"], a["x"], a["N"], a["y"], a["M"],
                        a["D"], a["sums"], a["xgrad"], a["ws"], a["wsb"], None)

  for bad in ({"spec": None}, {"x": None}, {"y": None}, {"sums": None}, {"ws": None}, {"D": 0}, {"D": 15}, {"N": 1},
              {"M": 1}, {"S": 0}, {"S": 65}, {"spec": spec(kind=2)}, {"spec": spec(kind=-1)}, {"spec": spec(bws=())},
              {"spec": spec(bws=(1.0,) * 9)}, {"spec": spec(bws=(1.0, 0.0))}, {"spec": spec(bws=(1.0, -2.0))},
              {"spec": spec(bws=(float("inf"),))}, {"spec": spec(bws=(float("nan"),))}, {"spec": spec(bws=(1e-30,))},
              {"wsb": nbytes.value - 8}, {"xgrad": None, "wsb": small.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import applications as app, solvers, utils
  from cnf_ot_amd.distributed import Shard
  x, y = np.zeros((5, 3), dtype=np.float32), np.ones((7, 3), dtype=np.float32)
  ok = dict(x=x, y=y, bandwidths=[1.0, 2.0])
  for bad in ({"x": x[:1]}, {"y": y[:1]}, {"bandwidths": [1.0] * 9}, {"bandwidths": []}, {"bandwidths": [1.0, -2.0]},
              {"bandwidths": [0.0]}, {"bandwidths": [float("nan")]}, {"bandwidths": [float("inf")]},
              {"y": np.ones((7, 2), dtype=np.float32)}, {"x": np.zeros((2, 5, 3)), "y": np.ones((3, 7, 3))},
              {"x": np.zeros((5, 15)), "y": np.ones((7, 15))}, {"x": np.zeros((65, 5, 3)), "y": np.ones((65, 7, 3))},
              {"x": np.zeros(5)}, {"kind": "laplace"}):
    with pytest.raises(ValueError):
      utils.mmd2(**dict(ok, **bad))
  with pytest.raises(ValueError):
    utils.median_bandwidths(np.zeros((1, 3)))
  with pytest.raises(ValueError):
    utils.median_bandwidths(np.zeros((8, 3)))      # (a median distance of 0 is no bandwidth)
  assert utils.MEDIAN_BANDWIDTH_FACTORS == (0.25, 0.5, 1.0, 2.0, 4.0)
  bw = utils.median_bandwidths(np.array([[0.0], [1.0], [3.0]]))      # pair distances 1, 2, 3 (torch: the lower median)
  assert bw == [0.25 * 2.0, 0.5 * 2.0, 2.0, 4.0, 8.0]
  # the training term: world > 1, a D mismatch, N < 2, a set count that is not the number of times, a bad bandwidth
  tgt = np.ones((130, 2), dtype=np.float32)
  with pytest.raises(ValueError):
    app.mmd_loss_fn(None, 2, None, tgt, [0.5], 0, 96, shard=Shard(0, 2))
  for kw in ({"target": np.ones((130, 3), dtype=np.float32)}, {"batch_size": 1}, {"target": np.ones((2, 130, 2))},
             {"bandwidths": [1.0] * 9}, {"bandwidths": [-1.0]}, {"kind": "laplace"}, {"target": tgt[:1]}):
    a = dict(dict(target=tgt, batch_size=96, bandwidths=None, kind="gaussian"), **kw)
    with pytest.raises(ValueError):
      app.mmd_loss_fn(None, 2, None, a["target"], [0.5], 0, a["batch_size"], bandwidths=a["bandwidths"], kind=a["kind"],
                      shard=Shard(0, 1))
  # the evaluation: wrong problem type, a configuration without figure settings, odd n_particles, times off the step
  for over in ({"general": {"type": "rwpo"}}, {"general": {"type": "ot"}}, {"general": {"type": "fp", "dim": 5}}):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_two_sample(solvers.load_config(overrides=over), None, None)
  fpc = solvers.load_config(overrides={"general": {"type": "fp"}})
  for kw in ({"n_particles": 4097}, {"n_particles": 2}, {"times": [0.0, 0.0005]}, {"bandwidths": [1.0] * 9},
             {"bandwidths": [1.0, -1.0]}):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_two_sample(fpc, None, None, **kw)
  assert solvers._parse(["--two-sample"]).two_sample and not solvers._parse([]).two_sample
  with pytest.raises(ValueError):      # (the checked-in default is rwpo: refused before any training step)
    solvers.main(solvers.load_config(), two_sample=True)
