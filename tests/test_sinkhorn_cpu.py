"""CPU tests of the Sinkhorn divergence: known answers of the float64 restatement (tests/sinkhorn_ref.py) the GPU tests
hold cnf_sinkhorn to, utils.sinkhorn_schedule, the host-side argument checks of cnf_sinkhorn through the C ABI (no device
is touched) and the Python entry points' refusals, which come before any device work.

Measured (every test prints its figures: run with -s):
  S(x, x), D = 2, N = 300                       value 0.0, largest |N xgrad| 0.0 (the x-y and x-x problems are one)
  translation, D = 2, N = 512, c = (1.5, -0.75) value error 1.6e-9 (bar 1e-6), N xgrad + c 9.4e-5 (bar 1e-3)
  translation, D = 1, N = 300, c = 1.5          value error 1.4e-9,            N xgrad + c 7.7e-5
  envelope gradient, D = 2, N = 40, M = 30      3.5e-10 against central differences on N grad of size 1.22 (bar 1e-5)
  Gaussian closed form, n = 1 024, eps = 0.1    2 S = 19.620 against W2^2 = 19.861: 1.2 % (bar 5 %)
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sinkhorn_ref as sr


def test_a_cloud_against_itself_is_zero():
  x, _ = sr.clouds(2, 300, 2, seed=1)
  r = sr.run(x, x.copy(), sr.schedule(x, x, 0.5, 0.5, 5))
  print(f"\n[sinkhorn S(x, x)] value {r['divergence']:.3e}, largest |N xgrad| {np.abs(r['xgrad']).max() * len(x):.3e}")
  # f and p (g and q) see the same numbers in the same order: their difference is rounding of a sum of N terms
  assert abs(r["divergence"]) <= 1e-17 * 300 and np.abs(r["xgrad"]).max() * len(x) <= 1e-17 * 300


@pytest.mark.parametrize("D,N,c", [(2, 512, (1.5, -0.75)), (1, 300, (1.5,))])
def test_translation(D, N, c):
  """y = x + c: the optimal plan is the shift for ANY eps, S_eps = |c|^2 / 2 and N xgrad = -c at convergence"""
  x, _ = sr.clouds(D, N, 2, seed=2 + D)
  x = x.astype(np.float64)
  c = np.array(c)
  y = x + c
  r = sr.run(x, y, sr.schedule(x, y, 0.5, 0.5, 60))
  e_v = abs(r["divergence"] - 0.5 * c @ c)
  e_g = float(np.abs(r["xgrad"] * N + c).max())
  print(f"\n[sinkhorn translation D={D}] value error {e_v:.2e}, N xgrad + c {e_g:.2e}, change {r['sums'][4]:.1e} {r['sums'][5]:.1e}")
  assert e_v <= 1e-6 and e_g <= 1e-3


def test_envelope_gradient_against_central_differences():
  D, N, M = 2, 40, 30
  x, y = sr.clouds(D, N, M, seed=7)
  x, y = x.astype(np.float64), y.astype(np.float64)
  sched = sr.schedule(x, y, 0.5, 0.8, 200)                # (one schedule for every perturbed run)
  g = sr.run(x, y, sched)["xgrad"] * N
  h, worst = 1e-5, 0.0
  for i in (0, 7, N - 1):
    for d in range(D):
      xp, xm = x.copy(), x.copy()
      xp[i, d] += h
      xm[i, d] -= h
      fd = (sr.run(xp, y, sched)["divergence"] - sr.run(xm, y, sched)["divergence"]) / (2.0 * h) * N
      worst = max(worst, abs(fd - g[i, d]))
  print(f"\n[sinkhorn envelope gradient] central differences: {worst:.2e} on N grad of size {np.abs(g).max():.2f}")
  assert worst <= 1e-5


def test_gaussian_closed_form():
  n, eps = 1024, 0.1
  rng = np.random.default_rng(11)
  A = np.array([[5.0, 1.0], [1.0, 0.5]])
  src = rng.standard_normal((n, 2)) @ np.linalg.cholesky(A).T - 3.0
  tgt = rng.standard_normal((n, 2))
  w2 = 18.0 + np.trace(A) + 2.0 - 2.0 * np.sqrt(np.linalg.eigvalsh(A)).sum()
  r = sr.run(src, tgt, sr.schedule(src, tgt, eps))
  print(f"\n[sinkhorn Gaussian] 2 S = {2 * r['divergence']:.3f} against W2^2 = {w2:.3f}: "
        f"{100 * abs(2 * r['divergence'] / w2 - 1):.1f} %, change {r['sums'][4]:.1e}")
  assert abs(w2 - 19.861) <= 1e-3
  assert abs(2.0 * r["divergence"] / w2 - 1.0) <= 0.05


def test_schedule():
  from cnf_ot_amd import utils
  x = np.array([[0.0, 0.0], [3.0, 0.0]], dtype=np.float32)
  y = np.array([[1.0, 4.0], [1.0, 1.0], [2.0, 2.0]], dtype=np.float32)
  s = utils.sinkhorn_schedule(x, y, 0.05, ratio=0.5, extra=3)        # the box is 3 x 4: diagonal^2 = 25
  n_geo = math.ceil(math.log(25.0 / 0.05) / math.log(2.0))
  assert len(s) == n_geo + 3 and s[0] == 25.0 and s[-3:] == [0.05] * 3
  assert all(b == a * 0.5 for a, b in zip(s[:n_geo - 1], s[1:n_geo])) and s[n_geo - 1] > 0.05 >= s[n_geo - 1] * 0.5
  assert all(a >= b for a, b in zip(s[:-1], s[1:]))
  assert s == sr.schedule(x, y, 0.05, 0.5, 3)
  # sets: one box over all of them; the defaults
  s3 = utils.sinkhorn_schedule(np.stack([x, x + 10.0]), np.stack([y, y]), 0.05)
  assert s3[0] == 13.0 ** 2 + 10.0 ** 2 and s3[-10:] == [0.05] * 10 and s3[1] == s3[0] * 0.8
  assert utils.sinkhorn_schedule(x, y, 100.0, extra=2) == [100.0, 100.0]
  # the cap: 512 entries are accepted, 513 are not
  assert len(utils.sinkhorn_schedule(x, y, 100.0, extra=512)) == 512
  for kw in ({"extra": 513, "eps": 100.0}, {"eps": 1e-30, "ratio": 0.9}, {"eps": 0.0}, {"eps": -1.0}, {"eps": float("nan")},
             {"ratio": 1.0}, {"ratio": 0.0}, {"extra": -1}, {"eps": 100.0, "extra": 0}):
    with pytest.raises(ValueError):
      utils.sinkhorn_schedule(x, y, **dict({"eps": 0.05}, **kw))
  assert utils.sinkhorn_check_schedule([0.5, 0.25]) == [0.5, 0.25]
  for bad in ([], [0.1] * 513, [0.1, 0.0], [-0.1], [float("inf")], [float("nan")], [1e-39], [1e39]):
    with pytest.raises(ValueError):
      utils.sinkhorn_check_schedule(bad)


def test_the_c_abi_refuses_before_the_device():
  """Every rejection of cnf_sinkhorn and cnf_sinkhorn_workspace comes back CNF_ERR_INVALID on a machine without a GPU;
  the buffers are host memory that no rejected call may read or write: they keep their fill."""
  from cnf_ot_amd import _capi
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_sinkhorn_workspace(3, 300, 257, 10, ctypes.byref(nbytes)) == _capi.CNF_OK
  P = lib.cnf_sinkhorn_splits(3, 300, 257, 10)
  W = 2 * (300 + 257)
  assert P >= 1 and nbytes.value == 3 * 3 * W * 4 + 3 * P * W * 4 + 3 * P * W * 8 + 3 * P * 2 * 300 * 10 * 8
  # the split count is a function of the sizes alone: 1 while the longer side is one tile of 64 columns
  assert lib.cnf_sinkhorn_splits(1, 64, 64, 2) == 1 and lib.cnf_sinkhorn_splits(1, 65, 64, 2) == 2
  assert lib.cnf_sinkhorn_splits(8, 2048, 2048, 2) == 16 and lib.cnf_sinkhorn_splits(5, 8192, 8192, 10) == 7
  small = ctypes.c_int64(-1)
  for bad in ((0, 300, 257, 10), (65, 300, 257, 10), (3, 1, 257, 10), (3, 300, 1, 10), (3, 300, 257, 0),
              (3, 300, 257, 15), (3, (1 << 20) + 1, 257, 2), (3, 300, (1 << 20) + 1, 2)):
    assert lib.cnf_sinkhorn_workspace(*bad, ctypes.byref(small)) == INV, bad
    assert lib.cnf_sinkhorn_splits(*bad) == INV, bad
  assert small.value == -1 and lib.cnf_sinkhorn_workspace(3, 300, 257, 10, None) == INV

  f32, f64 = np.full(3 * 300 * 10, 7.25, np.float32), np.full(18, 7.25, np.float64)
  ws = np.full(64, 7.25, np.float64)
  p, d, w = f32.ctypes.data, f64.ctypes.data, ws.ctypes.data
  good = dict(S=3, x=p, N=300, y=p, M=257, D=10, eps=[0.5, 0.25, 0.1], n=None, sums=d, pot=p, xgrad=p, xmap=p, ws=w,
              wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    eps = None if a["eps"] is None else (ctypes.c_double * max(len(a["eps"]), 1))(*a["eps"])
    n = len(a["eps"] or []) if a["n"] is None else a["n"]
    return lib.cnf_sinkhorn(a["S"], a["x"], a["N"], a["y"], a["M"], a["D"], eps, n, a["sums"], a["pot"], a["xgrad"], a["xmap"],
                            a["ws"], a["wsb"], None)

  bad = [{"x": None}, {"y": None}, {"eps": None, "n": 3}, {"sums": None}, {"ws": None}, {"S": 0}, {"S": 65}, {"D": 0}, {"D": 15},
         {"N": 1}, {"M": 1}, {"N": (1 << 20) + 1}, {"M": (1 << 20) + 1}, {"n": 0}, {"n": -1}, {"eps": [0.1] * 513},
         {"eps": [0.5, 0.0]}, {"eps": [0.5, -0.1]}, {"eps": [float("inf")]}, {"eps": [float("nan"), 0.1]}, {"eps": [1e-39]},
         {"eps": [1e39]}, {"wsb": nbytes.value - 8}, {"wsb": 0},
         {"pot": None, "xgrad": None, "xmap": None, "wsb": nbytes.value - 8}]
  wrong = {str(k): call(**k) for k in bad}
  wrong = {k: v for k, v in wrong.items() if v != INV}
  assert not wrong, wrong
  assert (f32 == 7.25).all() and (f64 == 7.25).all() and (ws == 7.25).all()


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import applications as app, solvers, utils
  from cnf_ot_amd.distributed import Shard
  x, y = np.zeros((5, 3), dtype=np.float32), np.ones((7, 3), dtype=np.float32)
  ok = dict(x=x, y=y, schedule=[0.5, 0.1])
  for bad in ({"x": x[:1]}, {"y": y[:1]}, {"schedule": []}, {"schedule": [0.1] * 513}, {"schedule": [0.1, -0.1]},
              {"schedule": [float("nan")]}, {"schedule": None, "eps": 0.0}, {"y": np.ones((7, 2), dtype=np.float32)},
              {"x": np.zeros((2, 5, 3)), "y": np.ones((3, 7, 3))}, {"x": np.zeros((5, 15)), "y": np.ones((7, 15))},
              {"x": np.zeros((65, 5, 3)), "y": np.ones((65, 7, 3))}, {"x": np.zeros(5)}):
    with pytest.raises(ValueError):
      utils.sinkhorn(**dict(ok, **bad))
  tgt = np.ones((130, 2), dtype=np.float32)
  with pytest.raises(ValueError):
    app.sinkhorn_loss_fn(None, 2, None, tgt, [0.5], 0, 96, shard=Shard(0, 2))
  for kw in ({"target": np.ones((130, 3), dtype=np.float32)}, {"batch_size": 1}, {"target": np.ones((2, 130, 2))},
             {"schedule": [0.1] * 513}, {"schedule": [-1.0]}, {"eps": 0.0}, {"target": tgt[:1]}):
    a = dict(dict(target=tgt, batch_size=96, eps=0.05, schedule=None), **kw)
    with pytest.raises(ValueError):
      app.sinkhorn_loss_fn(None, 2, None, a["target"], [0.5], 0, a["batch_size"], eps=a["eps"], schedule=a["schedule"],
                           shard=Shard(0, 1))
  for over in ({"general": {"type": "rwpo"}}, {"general": {"type": "fp"}}, {"general": {"type": "ot", "dim": 3}}):
    with pytest.raises(ValueError):
      solvers.evaluate_ot_reference(solvers.load_config(overrides=over), None, None)
  otc = solvers.load_config(overrides={"general": {"type": "ot", "dim": 2}})
  for kw in ({"n": 1}, {"n": (1 << 20) + 1}, {"eps": 0.0}, {"eps": float("nan")}):
    with pytest.raises(ValueError):
      solvers.evaluate_ot_reference(otc, None, None, **kw)
  assert solvers._parse(["--ot-reference"]).ot_reference and not solvers._parse([]).ot_reference
  with pytest.raises(ValueError):      # (the checked-in default is rwpo: refused before any training step)
    solvers.main(solvers.load_config(), ot_reference=True)
