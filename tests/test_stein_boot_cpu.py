"""CPU tests of the wild-bootstrap test of the kernel Stein discrepancy: the two float64 restatements of
tests/stein_boot_ref.py against each other (the direct definition q = 2 (S_A + S_B) - t on the subsets of every sign
vector, and the product form (E * (H E)).sum that cnf_stein_boot is built on), the sign words of utils.rademacher_signs,
the host-side refusals of the C ABI (no device is touched) and of the Python entry points, the condition on the inputs
that makes the GPU test's exact comparison of p-values fair, and the calibration of the bootstrap itself.

The two restatements: with H in float64, q, S_A, S_B and t are sums of at most N (N - 1) terms bounded by scale_v, each
formed to 1e-16 relative; the bound 1e-12 scale_v N (N - 1) on q leaves four orders of magnitude over what was seen
(up to 3.4e-17 scale_v N (N - 1)).

The p-value inputs (stein_boot_ref.P_VALUE_CASES, shared with tests/test_gpu_stein_boot.py): IMQ, c = 1, beta = -1/2,
D = 2, a standard normal cloud moved by a small shift against the score -x, 64 sign vectors of
rademacher_signs(sign_seed).  The value floor of the GPU bound is 4 EPS scale_v = 1.7e-4 and 1.4e-4; every null value
must lie farther than 4 floors from the observed one, so that an error within the bound on either side cannot change a
rank.  In the restatement: N = 96, cloud 1 moved by 0.15 under the signs of seed 4: min |null - observed| = 2.1e-3,
p = 18 / 64; N = 97, cloud 2 moved by 0.1 under the signs of seed 2: 2.1e-3, p = 25 / 64.

The calibration: 40 sets of exact N(0, I) draws, D = 2, N = 96, against -x, 63 sign vectors: the p-values are uniform,
so their mean lies within 0.5 +- 0.15 (the mean of 40 uniform values has sd 0.046: a 3.3 sd band) and at most 6 of 40
fall below 0.05 (expected 2; 6 or fewer with probability 0.997).  Seen here (sets of stein_ref.cloud(seed 9000 + k)):
mean 0.452, 3 of 40; the float64 run that chose the test, on other draws: mean 0.53, 1 of 40.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stein_boot_ref as br
import stein_ref as sr

EPS = br.EPS
P_VALUE_CASES, p_value_inputs = br.P_VALUE_CASES, br.p_value_inputs


def _sp(kind):
  return (sr.spec("imq", [0.8, 1.7], [1.0, 0.5], beta=-0.75) if kind == "imq" else sr.spec("gaussian", [0.8, 1.7, 3.0]))


@pytest.mark.parametrize("kind", ["imq", "gaussian"])
@pytest.mark.parametrize("D,N", [(2, 37), (3, 20), (1, 2)])
def test_the_two_restatements_agree(D, N, kind):
  from cnf_ot_amd import utils
  x = sr.cloud(D, N, 11 + D)
  s = br.linear_score(x, 21 + D)
  sp = _sp(kind)
  plus = br.unpack(utils.rademacher_signs(N, 31, seed=2).numpy()).copy()
  # |A| = N (vector 0, as drawn), 0, 1 and N - 1
  plus[:, 5] = False
  plus[:, 6] = np.arange(N) == 1
  plus[:, 7] = np.arange(N) != N - 1
  assert plus[:, 0].all() and [int(plus[:, p].sum()) for p in (5, 6, 7)] == [0, 1, N - 1]
  direct = br.stats(x, s, sp, plus)
  q = br.q_product(br.kernel_matrix(x, s, sp), plus)
  pairs = N * (N - 1.0)
  err = float(np.abs(direct["q"] - q).max())
  print(f"[stein_boot restatements {kind} D={D} N={N}] {err:.2e} against {1e-12 * direct['scale_v'] * pairs:.2e}")
  assert err <= 1e-12 * direct["scale_v"] * pairs
  # vector 0 and the empty A are the statistic itself; one point moved across is t less four times its row
  assert direct["q"][0] == direct["t"] == direct["q"][5]
  assert np.allclose(direct["stats"][0], sr.ksd2(x, s, sp)[0], rtol=0.0, atol=1e-13 * direct["scale_v"])
  if N > 2:
    assert len({round(float(v), 9) for v in direct["q"]}) > 20     # (the vectors differ, and so do their values)


@pytest.mark.parametrize("N,n_boot", [(5, 31), (96, 63), (300, 255)])
def test_rademacher_signs(N, n_boot):
  from cnf_ot_amd import utils
  words = utils.rademacher_signs(N, n_boot, seed=3)
  assert words.dtype == torch.int32 and tuple(words.shape) == (N, (n_boot + 1) // 32) and not words.is_cuda
  plus = br.unpack(words.numpy())
  assert plus.shape == (N, n_boot + 1) and plus[:, 0].all()        # vector 0: all +1, the observed statistic
  assert torch.equal(words, utils.rademacher_signs(N, n_boot, seed=3))
  assert not torch.equal(words, utils.rademacher_signs(N, n_boot, seed=4))
  # fair bits: the count of +1 over the N n_boot drawn bits within 5 standard deviations of its mean
  bits = N * n_boot
  assert abs(int(plus[:, 1:].sum()) - 0.5 * bits) <= 5.0 * 0.5 * np.sqrt(bits)
  assert len({plus[:, p].tobytes() for p in range(n_boot + 1)}) > n_boot // 2 or N < 8      # (the vectors differ)
  # the bit layout is two_sample.pack_labels': the words written bit by bit from the signs are the same
  assert np.array_equal(br.pack(plus), words.numpy()) and torch.equal(utils.pack_labels(plus), words)


def test_rademacher_signs_refusals():
  from cnf_ot_amd import utils
  for n_boot in (0, 30, 32, 62, 1024, 1055, -1):
    with pytest.raises(ValueError):
      utils.rademacher_signs(10, n_boot)
  with pytest.raises(ValueError):
    utils.rademacher_signs(0, 31)
  assert tuple(utils.rademacher_signs(3, 1023).shape) == (3, 32)


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi, utils
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_stein_boot_workspace(3, 300, 10, 64, ctypes.byref(nbytes)) == _capi.CNF_OK
  SPL = lib.cnf_stein_boot_splits(3, 300, 10)
  groups = -(-300 // 64) * SPL                     # 64 rows per workgroup
  assert SPL >= 1 and nbytes.value == 8 * 3 * groups * (64 + 2)
  # the split count is a function of the sizes alone: 1 while the set is one tile of 64 columns
  assert lib.cnf_stein_boot_splits(1, 64, 2) == 1 and lib.cnf_stein_boot_splits(1, 65, 2) == 2
  for bad in ((0, 300, 10), (65, 300, 10), (3, 1, 10), (3, (1 << 20) + 1, 10), (3, 300, 0), (3, 300, 15)):
    assert lib.cnf_stein_boot_workspace(*bad, 64, ctypes.byref(nbytes)) == _capi.CNF_ERR_INVALID, bad
    assert lib.cnf_stein_boot_splits(*bad) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_stein_boot_splits(1, 1 << 20, 2) == 1
  for P in (0, 16, 33, 48, 1056, -32):
    assert lib.cnf_stein_boot_workspace(3, 300, 10, P, ctypes.byref(nbytes)) == _capi.CNF_ERR_INVALID, P
  assert lib.cnf_stein_boot_workspace(3, 300, 10, 64, None) == _capi.CNF_ERR_INVALID
  assert lib.cnf_stein_boot_workspace(3, 300, 10, 64, ctypes.byref(nbytes)) == _capi.CNF_OK

  def spec(**kw):
    sp = utils.stein_spec("imq", [1.0, 2.0])
    for k, v in kw.items():
      if isinstance(v, tuple):
        getattr(sp, k)[v[0]] = v[1]
      else:
        setattr(sp, k, v)
    return sp

  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  good = dict(spec=spec(), S=3, x=4096, score=8192, N=300, D=10, signs=12288, P=64, stats=16384, raw=20480, ws=24576,
              wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_stein_boot(None if a["spec"] is None else ctypes.byref(a["spec"]), a["S"], a["x"], a["score"], a["N"],
                              a["D"], a["signs"], a["P"], a["stats"], a["raw"], a["ws"], a["wsb"], None)

  inf, nan = float("inf"), float("nan")
  for bad in ({"spec": None}, {"x": None}, {"score": None}, {"signs": None}, {"stats": None}, {"ws": None}, {"D": 0},
              {"D": 15}, {"N": 1}, {"N": (1 << 20) + 1}, {"S": 0}, {"S": 65}, {"P": 0}, {"P": 16}, {"P": 48}, {"P": 1056},
              {"spec": spec(kind=0)}, {"spec": spec(kind=3)}, {"spec": spec(n_terms=0)}, {"spec": spec(n_terms=5)},
              {"spec": spec(w=(1, 0.0))}, {"spec": spec(w=(1, -1.0))}, {"spec": spec(w=(0, inf))}, {"spec": spec(w=(0, nan))},
              {"spec": spec(bw=(1, 0.0))}, {"spec": spec(bw=(0, -1.0))}, {"spec": spec(bw=(0, inf))},
              {"spec": spec(bw=(0, nan))}, {"spec": spec(beta=0.0)}, {"spec": spec(beta=-1.0)}, {"spec": spec(beta=nan)},
              {"spec": spec(bw=(0, 1e-9))}, {"spec": spec(bw=(0, 1e25))}, {"spec": spec(w=(0, 3e38))},
              {"spec": spec(kind=2, bw=(0, 1e-7))}, {"wsb": nbytes.value - 8}, {"raw": None, "wsb": nbytes.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import solvers, utils
  utils.stein_boot_check_shapes((3, 300, 10))
  utils.stein_boot_check_shapes((3, 300, 10), (3, 300, 10), (300, 2))
  for bad in (((0, 300, 10),), ((65, 300, 10),), ((3, 1, 10),), ((3, (1 << 20) + 1, 10),), ((3, 300, 0),), ((3, 300, 15),),
              ((3, 300, 10), (3, 299, 10)), ((3, 300, 10), (2, 300, 10)), ((3, 300, 10), (3, 300, 9)),
              ((3, 300, 10), None, (299, 2)), ((3, 300, 10), None, (300, 0)), ((3, 300, 10), None, (300, 33)),
              ((3, 300, 10), None, (300,))):
    with pytest.raises(ValueError):
      utils.stein_boot_check_shapes(*bad)
  x = np.zeros((5, 3), dtype=np.float32)
  ok = dict(x=x, score=-x, bandwidths=[1.0, 2.0], n_boot=31)
  for bad in ({"x": x[:1], "score": -x[:1]}, {"score": -x[:4]}, {"score": np.zeros((5, 2), dtype=np.float32)},
              {"bandwidths": [1.0] * 5}, {"bandwidths": [-1.0]}, {"kind": "laplace"}, {"beta": 0.0}, {"weights": [1.0]},
              {"n_boot": 30}, {"n_boot": 1055}, {"x": np.zeros((2, 5, 3)), "score": np.zeros((3, 5, 3))}, {"x": np.zeros(5)},
              {"x": np.zeros((5, 15)), "score": np.zeros((5, 15))},
              {"signs": torch.zeros(4, 1, dtype=torch.int32)}, {"signs": torch.zeros(5, 1, dtype=torch.int64)},
              {"signs": torch.zeros(5, 33, dtype=torch.int32)}):
    with pytest.raises(ValueError):
      utils.ksd_bootstrap_test(**dict(ok, **bad))
  cfg = solvers.load_config(overrides={"general": {"type": "fp"}})
  for kw in ({"n": 1}, {"n": (1 << 20) + 1}, {"kind": "laplace"}, {"n_boot": 254}, {"n_boot": 2047}):
    with pytest.raises(ValueError):
      solvers.evaluate_ksd_test(cfg, None, None, **kw)
  assert solvers._parse(["--ksd-test"]).ksd_test and not solvers._parse([]).ksd_test
  assert "stationary" not in solvers.KSD_TEST_ROWS


@pytest.mark.parametrize("case", P_VALUE_CASES, ids=lambda c: "cloud%d-signs%d" % (c["cloud_seed"], c["sign_seed"]))
def test_the_p_value_inputs_keep_every_null_value_away_from_the_observed_one(case):
  x, s, sp, words = p_value_inputs(case)
  assert sp["kind"] == "imq" and case["D"] == 2 and abs(case["N"] - 96) <= 1
  ref = br.stats(x, s, sp, br.unpack(words.numpy()))
  st = ref["stats"]
  floor = 4.0 * EPS * ref["scale_v"]
  gap = float(np.abs(st[1:] - st[0]).min())
  p = br.p_value(st[0], st[1:])
  print(f"[stein_boot p-value inputs] observed {st[0]:.4e}, min |null - observed| {gap:.2e} against a floor of {floor:.1e}, "
        f"p = {p * len(st):.0f} / {len(st)}")
  assert len(st) == 64
  assert gap > 4.0 * floor
  assert p == case["p"] and 1.0 / 64.0 < p < 1.0     # (a rank inside the null: the comparison is of a count, not of its floor)


def test_the_bootstrap_is_calibrated_on_exact_draws():
  from cnf_ot_amd import utils
  D, N, sets = 2, 96, 40
  sp = sr.spec("imq", [1.0])
  plus = br.unpack(utils.rademacher_signs(N, 63, seed=0).numpy())
  ps = []
  for k in range(sets):
    x = sr.cloud(D, N, 9000 + k)
    st = br.stats(x, -x, sp, plus)["stats"]
    ps.append(br.p_value(st[0], st[1:]))
  ps = np.array(ps)
  print(f"[stein_boot calibration] mean p {ps.mean():.3f}, {int((ps < 0.05).sum())} of {sets} below 0.05, min {ps.min():.3f}")
  assert abs(ps.mean() - 0.5) <= 0.15
  assert int((ps < 0.05).sum()) <= 6
