"""The nearest-neighbour estimators without a device: the float64 restatement (tests/knn_ref.py) against closed forms,
utils.knn_estimates against the restatement, and what cnf_knn and its Python surface refuse before any device work.

Closed forms, x ~ N(0, I), y ~ N(0.5 1, 1.25^2 I):  H = (D / 2) log(2 pi e),
KL(x || y) = D (log 1.25 + (1 + 0.25) / (2 * 1.5625) - 1 / 2).  The bounds of the closed-form test are the restatement's
own worst error over the test's seeds, times 2 (printed: run with -s); a bound above 0.1 nats would mean the restatement
is wrong, and is refused.  At D = 10 the estimator is biased upwards (KL by +0.17 .. +0.31 against 1.231 at N = 4 096):
the test pins the sign and the size, which is what evaluate_fp_knn's kl_floor column is for.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as kr

N_CLOSED, K = 4096, 4
SEEDS = (0, 1, 2)


def _closed_forms(D):
  return 0.5 * D * math.log(2.0 * math.pi * math.e), D * (math.log(1.25) + (1.0 + 0.25) / (2.0 * 1.5625) - 0.5)


def _errors(D, seed):
  """(entropy error, KL error) of the restatement at rank K against the closed forms"""
  x = kr.gaussian(D, N_CLOSED, 100 + 10 * D + seed)
  y = kr.gaussian(D, N_CLOSED, 200 + 10 * D + seed, mean=0.5, scale=1.25)
  est = kr.estimates_of_clouds(x, y, K)
  H, KL = _closed_forms(D)
  return est["entropy"][-1] - H, est["kl"][-1] - KL


def test_the_restatement_against_closed_forms():
  errs = np.array([[_errors(D, seed) for seed in SEEDS] for D in (1, 2, 3)])      # [D, seed, (H, KL)]
  bound_h, bound_kl = 2.0 * np.abs(errs[..., 0]).max(), 2.0 * np.abs(errs[..., 1]).max()
  print(f"\n[knn closed forms] H error {errs[..., 0].min():+.4f} .. {errs[..., 0].max():+.4f} (bound {bound_h:.4f}), "
        f"KL error {errs[..., 1].min():+.4f} .. {errs[..., 1].max():+.4f} (bound {bound_kl:.4f})")
  assert bound_h <= 0.1 and bound_kl <= 0.1, "the restatement is wrong, not the bound"
  assert (np.abs(errs[..., 0]) <= bound_h).all() and (np.abs(errs[..., 1]) <= bound_kl).all()


def test_the_dimension_10_bias_has_its_sign_and_size():
  eh, ekl = _errors(10, 0)
  print(f"\n[knn D=10] H error {eh:+.4f}, KL bias {ekl:+.4f} against {_closed_forms(10)[1]:.4f}")
  assert 0.0 < ekl < 0.5
  assert abs(eh) < 0.5


def _small_sums(seed=5, D=1, N=60, M=45, k=6):
  x, y = kr.exact_grid(D, N, seed), kr.exact_grid(D, M, seed + 1)      # (a grid cloud: some distances are 0)
  return np.stack([kr.sums_of(kr.neighbours(x, None, k)[0]), kr.sums_of(kr.neighbours(x, y, k)[0])]), N, M, D


def test_knn_estimates_is_the_restatements_estimators():
  from cnf_ot_amd import utils
  sums, N, M, D = _small_sums()
  assert sums[:, :, 1].sum() > 0
  got = utils.knn_estimates(torch.from_numpy(np.stack([sums, sums])), N, M, D)
  want = kr.estimates(sums, N, M, D)
  for key in ("entropy", "cross_entropy", "kl"):
    assert got[key].dtype == torch.float64 and got[key].shape == (2, sums.shape[1])
    assert np.abs(got[key][0].numpy() - want[key]).max() <= 1e-12, key
  assert np.array_equal(got["zeros"][0].numpy(), sums[:, :, 1])
  alone = utils.knn_estimates(torch.from_numpy(sums[None]), N, 0, D)
  assert alone["kl"] is None and alone["cross_entropy"] is None
  assert np.abs(alone["entropy"][0].numpy() - want["entropy"]).max() <= 1e-12
  # a large N: psi from torch.special.digamma against the harmonic sum
  big = utils.knn_estimates(torch.from_numpy(sums[None]), 1 << 20, 1 << 19, D)
  ref = kr.estimates(sums, 1 << 20, 1 << 19, D)
  assert np.abs(big["kl"][0].numpy() - ref["kl"]).max() <= 1e-12 and np.abs(big["entropy"][0].numpy() - ref["entropy"]).max() <= 1e-12


def test_entropy_of_a_scaled_cloud():
  D, N, k, a = 3, 300, 5, 4.0                              # (a power of two: the scaled cloud is exact in float32)
  x = kr.gaussian(D, N, 7)
  h = kr.estimates(np.stack([kr.sums_of(kr.neighbours(x, None, k)[0])] * 2), N, 0, D)["entropy"]
  ha = kr.estimates(np.stack([kr.sums_of(kr.neighbours(a * x, None, k)[0])] * 2), N, 0, D)["entropy"]
  assert np.abs(ha - h - D * math.log(a)).max() <= 1e-12


def _c_call(lib, S=1, N=8, M=6, D=2, k=4, x=True, y=True, sums=True, ws=True, dxy=False, short=0, buf=None):
  """cnf_knn on HOST buffers that a refused call must neither read nor write"""
  nbytes = ctypes.c_int64(0)
  lib.cnf_knn_workspace(1, 64, 64, 2, 16, ctypes.byref(nbytes))
  have = nbytes.value
  if lib.cnf_knn_workspace(S, N, M, D, k, ctypes.byref(nbytes)) == 0:
    have = nbytes.value - short
  p = buf.ctypes.data
  return lib.cnf_knn(S, p if x else None, N, p if y else None, M, D, k, None, None, p if dxy else None, None,
                     p if sums else None, p if ws else None, have, None)


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  buf = np.full(1 << 16, 7.25, np.float64)
  nbytes = ctypes.c_int64(-1)
  q = lambda *a: lib.cnf_knn_workspace(*a, ctypes.byref(nbytes))
  bad = {
      "k=0": dict(k=0), "k=17": dict(k=17, N=64, M=64), "N=k": dict(N=4), "M=k-1": dict(M=3),
      "D=0": dict(D=0), "D=15": dict(D=15), "S=0": dict(S=0), "S=65": dict(S=65), "N=2^20+1": dict(N=(1 << 20) + 1),
      "M=2^20+1": dict(M=(1 << 20) + 1),
  }
  for tag, kw in bad.items():
    args = dict(S=1, N=8, M=6, D=2, k=4)
    args.update(kw)
    assert q(args["S"], args["N"], args["M"], args["D"], args["k"]) == INV and nbytes.value == -1, tag
    assert _c_call(lib, buf=buf, **kw) == INV, tag
  assert q(1, 8, 6, 2, 4) == 0 and nbytes.value > 0
  assert lib.cnf_knn_workspace(1, 8, 6, 2, 4, None) == INV
  assert q(1, 8, 0, 2, 4) == 0                             # (M = 0: the self block alone)
  for tag, kw in {"x NULL": dict(x=False), "sums NULL": dict(sums=False), "workspace NULL": dict(ws=False),
                  "y NULL, M != 0": dict(y=False), "y given, M == 0": dict(M=0), "dist_xy given, M == 0": dict(M=0, y=False, dxy=True),
                  "a short workspace": dict(short=1)}.items():
    assert _c_call(lib, buf=buf, **kw) == INV, tag
  assert (buf == 7.25).all()
  assert lib.cnf_knn_splits(1, 8, 6, 2) == 1 and lib.cnf_knn_splits(1, 8, 0, 2) == 1
  for a in ((0, 8, 6, 2), (65, 8, 6, 2), (1, 8, 6, 0), (1, 8, 6, 15), (1, (1 << 20) + 1, 6, 2), (1, 8, (1 << 20) + 1, 2), (1, 1, 6, 2)):
    assert lib.cnf_knn_splits(*a) == INV, a


def test_the_workspace_grows_with_k():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  nbytes, last = ctypes.c_int64(0), 0
  for k in range(1, 17):
    assert lib.cnf_knn_workspace(3, 700, 1100, 2, k, ctypes.byref(nbytes)) == 0
    assert nbytes.value > last and nbytes.value % 8 == 0
    last = nbytes.value


def test_the_python_surface_refuses_before_the_device():
  from cnf_ot_amd import utils
  z = lambda *shape: torch.zeros(*shape)
  bad = {
      "k=0": (z(8, 2), z(6, 2), 0), "k=17": (z(64, 2), z(64, 2), 17), "N=k": (z(4, 2), z(6, 2), 4), "M=k-1": (z(8, 2), z(3, 2), 4),
      "D=0": (z(8, 0), z(6, 0), 4), "D=15": (z(8, 15), z(6, 15), 4), "S=0": (z(0, 8, 2), z(0, 6, 2), 4),
      "S=65": (z(65, 8, 2), z(65, 6, 2), 4), "N=2^20+1": (z((1 << 20) + 1, 1), z(6, 1), 4), "S differs": (z(2, 8, 2), z(3, 6, 2), 4),
      "D differs": (z(8, 2), z(6, 3), 4), "a 1-D x": (z(8), z(6, 2), 4), "N=k, no y": (z(4, 2), None, 4),
  }
  for tag, (x, y, k) in bad.items():
    with pytest.raises(ValueError):
      utils.knn(x, y, k)
    if y is not None:
      with pytest.raises(ValueError):
        utils.knn_divergence(x, y, k)
    else:
      with pytest.raises(ValueError):
        utils.knn_entropy(x, k)
  with pytest.raises(ValueError):
    utils.knn_check_shapes((1, 8, 2), (1, 6, 2), 7)        # M < k
  utils.knn_check_shapes((1, 8, 2), (1, 7, 2), 7)
  utils.knn_check_shapes((64, 1 << 20, 14), None, 16)


def test_evaluate_fp_knn_refuses_before_the_device():
  from cnf_ot_amd import solvers
  assert solvers._parse(["--knn"]).knn and not solvers._parse([]).knn
  cfg = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}})
  with pytest.raises(ValueError):
    solvers.evaluate_fp_knn(cfg, None, None, n_particles=4096, k=17)
  with pytest.raises(ValueError):
    solvers.evaluate_fp_knn(cfg, None, None, n_particles=8, k=4)       # halves of 4 points: N = k
  with pytest.raises(ValueError):
    solvers.evaluate_fp_knn(cfg, None, None, n_particles=4097)
  with pytest.raises(ValueError):
    solvers.evaluate_fp_knn(solvers.load_config(), None, None)         # rwpo
  with pytest.raises(ValueError):
    solvers.main(solvers.load_config(), epochs=0, knn=True)


@pytest.mark.parametrize("case", kr.GAUSSIAN_CASES, ids=lambda c: "D%d-N%d-M%d" % c)
def test_the_index_rule_leaves_out_at_most_one_percent(case):
  """The rule of the GPU test -- compare an index only where the restatement's distance is further than twice the float32
  bound from both neighbouring ranks -- computed on that test's own clouds with the restatement alone"""
  D = case[0]
  for k in kr.GAUSSIAN_KS:
    for block, (d2, _) in zip(("self", "cross"), kr.gaussian_reference(*case, k)):
      keep = kr.index_rule(d2, k, kr.distance_bound(D))
      left_out = 1.0 - keep.mean()
      print(f"\n[knn index rule D={D} k={k} {block}] left out {left_out:.2e} of {keep.size}")
      assert left_out <= 0.01
