"""CPU tests of the permutation test of the kernel two-sample statistics: the label words of utils.permutation_labels,
the identity q, r, t -> statistic that cnf_mmd_perm is built on against the direct definition (tests/mmd_perm_ref.py:
mmd_ref.mmd2 on the two subsets of every label vector), the p-value formula, the host-side refusals of the C ABI (no
device is touched) and of the Python entry points, and the condition on the inputs that makes the GPU test's exact
comparison of p-values fair.

The identity: with K in float64, q, r, t and the block sums are sums of n^2 terms bounded by k_max, each formed to
1e-16 relative; the bound 1e-12 k_max on the statistic leaves four orders of magnitude over what was seen (up to 2e-15).

The p-value inputs (mmd_perm_ref.P_VALUE_CASES, shared with tests/test_gpu_mmd_perm.py): D = 2, N = 96, M = 80,
mmd_ref.clouds(seed, shift=0.25, scale=1.0), three bandwidths sqrt(D) 0.5 2^b, 64 label vectors of
permutation_labels(label_seed).  The value floor of the GPU bound is 4 eps k_max = 6e-5; every null value must lie
farther than 4 floors from the observed one, so that an error within the bound on either side cannot change a rank.  In
the restatement: clouds of seed 5 under the labels of seed 1, the observed value in the null's tail: min |null -
observed| = 1.4e-2, p = 3 / 64; clouds of seed 8 under the labels of seed 3, the observed value in the middle of the
null: min |null - observed| = 9.2e-4, p = 28 / 64.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_perm_ref as pr
import mmd_ref as mr

EPS = pr.EPS
P_VALUE_CASES, p_value_inputs = pr.P_VALUE_CASES, pr.p_value_inputs


@pytest.mark.parametrize("N,M,n_perm", [(5, 3, 31), (96, 80, 63), (40, 70, 255)])
def test_permutation_labels(N, M, n_perm):
  from cnf_ot_amd import utils
  words = utils.permutation_labels(N, M, n_perm, seed=3)
  assert words.dtype == torch.int32 and tuple(words.shape) == (N + M, (n_perm + 1) // 32) and not words.is_cuda
  member = pr.unpack(words.numpy())
  assert member.shape == (N + M, n_perm + 1)
  assert member[:N, 0].all() and not member[N:, 0].any()          # vector 0: the identity labelling
  assert (member.sum(0) == N).all()                                # every vector: exactly N points in the first sample
  assert torch.equal(words, utils.permutation_labels(N, M, n_perm, seed=3))
  assert not torch.equal(words, utils.permutation_labels(N, M, n_perm, seed=4))
  assert len({member[:, p].tobytes() for p in range(n_perm + 1)}) > n_perm // 2      # (the vectors differ)
  # the bit layout: the words written bit by bit from the membership are the same, and so are pack_labels'
  assert np.array_equal(pr.pack(member), words.numpy())
  assert torch.equal(utils.pack_labels(member), words)
  # one bit alone: vector 37 of point 2 is bit 5 of word 1
  one = np.zeros((4, 64), dtype=bool)
  one[2, 37] = True
  w = utils.pack_labels(one).numpy().view(np.uint32)
  assert w[2, 1] == 1 << 5 and w.sum() == 1 << 5
  # bit 31 is the sign bit of the int32 word
  top = np.zeros((1, 32), dtype=bool)
  top[0, 31] = True
  assert int(utils.pack_labels(top)[0, 0]) == -(1 << 31) and pr.unpack(utils.pack_labels(top).numpy())[0, 31]


def test_permutation_labels_refusals():
  from cnf_ot_amd import utils
  for n_perm in (0, 30, 32, 62, 1024, 1055, -1):
    with pytest.raises(ValueError):
      utils.permutation_labels(10, 10, n_perm)
  with pytest.raises(ValueError):
    utils.permutation_labels(0, 10, 31)
  with pytest.raises(ValueError):
    utils.pack_labels(np.zeros((4, 33), dtype=bool))
  assert tuple(utils.permutation_labels(3, 3, 1023).shape) == (6, 32)


@pytest.mark.parametrize("kind", ["gaussian", "energy"])
@pytest.mark.parametrize("D,N,M", [(2, 37, 29), (3, 20, 45), (1, 2, 2)])
def test_the_identity_against_the_direct_definition(D, N, M, kind):
  from cnf_ot_amd import utils
  x, y = mr.clouds(D, N, M, seed=11 + D)
  sp = mr.spec(kind, [0.8, 1.7, 3.0] if kind == "gaussian" else ())
  member = pr.unpack(utils.permutation_labels(N, M, 31, seed=2).numpy()).copy()
  # other counts than N: vector 5 moves a point across, vector 6 three; (N = M = 2: a vector with one point, NaN)
  member[N, 5] = True
  member[:3, 6] = ~member[:3, 6]
  member[:, 7] = False
  member[0, 7] = True
  direct = pr.stats(x, y, sp, member)
  q, r, t = pr.qrt(pr.kernel_matrix(x, y, sp), member)
  ident = pr.stats_of_qrt(q, r, t, member.sum(0), N + M)
  assert np.isnan(direct[7]) and np.isnan(ident[7]) and np.array_equal(np.isnan(direct), np.isnan(ident))
  ok = ~np.isnan(direct)
  assert ok.sum() >= 24 or (N, M) == (2, 2)
  err = float(np.abs(direct[ok] - ident[ok]).max())
  k_max = mr.k_max(x, y, sp)
  print(f"[mmd_perm identity {kind} D={D} N={N} M={M}] {err:.2e} (k_max {k_max:.3g})")
  assert err <= 1e-12 * k_max
  assert direct[0] == mr.mmd2(x, y, sp)                            # vector 0 is the two samples as given


def test_p_value_formula():
  from cnf_ot_amd import utils
  null = [0.1, 0.5, 0.5, 0.9, -0.2, 0.3, 0.0]
  for obs, want in ((1.0, 1 / 8), (0.9, 2 / 8), (0.5, 4 / 8), (0.4, 4 / 8), (-0.2, 8 / 8), (-1.0, 8 / 8), (0.0, 7 / 8)):
    assert pr.p_value(obs, np.array(null)) == want
    got = utils.permutation_p_value(torch.tensor([obs, obs], dtype=torch.float64), torch.tensor([null, null], dtype=torch.float64))
    assert got.dtype == torch.float64 and got.tolist() == [want, want]
  # per set: each row against its own observed value
  got = utils.permutation_p_value(torch.tensor([0.5, 2.0], dtype=torch.float64),
                                  torch.tensor([[0.5, 0.6, 0.4], [1.0, 1.5, 1.9]], dtype=torch.float64))
  assert got.tolist() == [3 / 4, 1 / 4]


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_mmd_perm_workspace(3, 300, 257, 10, 64, ctypes.byref(nbytes)) == _capi.CNF_OK
  SPL = lib.cnf_mmd_perm_splits(3, 300, 257, 10)
  groups = -(-557 // 64) * SPL                     # 64 pooled rows per workgroup
  assert SPL >= 1 and nbytes.value == 8 * 3 * groups * (2 * 64 + 1) + 4 * 64
  # the split count is a function of the sizes alone: 1 while the pooled sample is one tile of 64 columns
  assert lib.cnf_mmd_perm_splits(1, 32, 32, 2) == 1 and lib.cnf_mmd_perm_splits(1, 33, 32, 2) == 2
  for bad in ((0, 300, 257, 10), (65, 300, 257, 10), (3, 1, 257, 10), (3, 300, 1, 10), (3, 300, 257, 0), (3, 300, 257, 15),
              (1, 1 << 19, (1 << 19) + 1, 2)):
    assert lib.cnf_mmd_perm_workspace(*bad, 64, ctypes.byref(nbytes)) == _capi.CNF_ERR_INVALID, bad
    assert lib.cnf_mmd_perm_splits(*bad) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_mmd_perm_splits(1, 1 << 19, 1 << 19, 2) == 1
  for P in (0, 16, 33, 48, 1056, -32):
    assert lib.cnf_mmd_perm_workspace(3, 300, 257, 10, P, ctypes.byref(nbytes)) == _capi.CNF_ERR_INVALID, P
  assert lib.cnf_mmd_perm_workspace(3, 300, 257, 10, 64, None) == _capi.CNF_ERR_INVALID
  assert lib.cnf_mmd_perm_workspace(3, 300, 257, 10, 64, ctypes.byref(nbytes)) == _capi.CNF_OK

  def spec(kind=0, bws=(1.0, 2.0)):
    s = _capi.CnfMmdSpec()
    s.kind, s.n_bw = kind, len(bws)
    for i, b in enumerate(bws[:8]):
      s.bw[i] = b
    return s

  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  good = dict(spec=spec(), S=3, x=4096, N=300, y=8192, M=257, D=10, labels=12288, P=64, stats=16384, raw=20480, ws=24576,
              wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_mmd_perm(None if a["spec"] is None else ctypes.byref(a["spec"]), a["S"], a["x"], a["N"], a["y"], a["M"],
                            a["D"], a["labels"], a["P"], a["stats"], a["raw"], a["ws"], a["wsb"], None)

  for bad in ({"spec": None}, {"x": None}, {"y": None}, {"labels": None}, {"stats": None}, {"ws": None}, {"D": 0}, {"D": 15},
              {"N": 1}, {"M": 1}, {"S": 0}, {"S": 65}, {"N": 1 << 20}, {"P": 0}, {"P": 48}, {"P": 1056},
              {"spec": spec(kind=2)}, {"spec": spec(kind=-1)}, {"spec": spec(bws=())}, {"spec": spec(bws=(1.0,) * 9)},
              {"spec": spec(bws=(1.0, 0.0))}, {"spec": spec(bws=(1.0, -2.0))}, {"spec": spec(bws=(float("inf"),))},
              {"spec": spec(bws=(float("nan"),))}, {"spec": spec(bws=(1e-30,))}, {"wsb": nbytes.value - 8},
              {"raw": None, "wsb": nbytes.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import solvers, utils
  utils.mmd_perm_check_shapes((3, 300, 10), (3, 257, 10))
  utils.mmd_perm_check_shapes((3, 300, 10), (3, 257, 10), (557, 2))
  for bad in (((0, 300, 10), (0, 257, 10)), ((65, 300, 10), (65, 257, 10)), ((3, 1, 10), (3, 257, 10)),
              ((3, 300, 10), (3, 1, 10)), ((3, 300, 10), (3, 257, 9)), ((3, 300, 10), (2, 257, 10)),
              ((3, 300, 15), (3, 257, 15)), ((1, 1 << 19, 2), (1, (1 << 19) + 1, 2)),
              ((3, 300, 10), (3, 257, 10), (556, 2)), ((3, 300, 10), (3, 257, 10), (557, 0)),
              ((3, 300, 10), (3, 257, 10), (557, 33)), ((3, 300, 10), (3, 257, 10), (557,))):
    with pytest.raises(ValueError):
      utils.mmd_perm_check_shapes(*bad)
  x, y = np.zeros((5, 3), dtype=np.float32), np.ones((7, 3), dtype=np.float32)
  ok = dict(x=x, y=y, bandwidths=[1.0, 2.0], n_perm=31)
  for bad in ({"x": x[:1]}, {"y": y[:1]}, {"bandwidths": [1.0] * 9}, {"bandwidths": [-1.0]}, {"kind": "laplace"},
              {"n_perm": 30}, {"n_perm": 1055}, {"y": np.ones((7, 2), dtype=np.float32)},
              {"x": np.zeros((2, 5, 3)), "y": np.ones((3, 7, 3))}, {"x": np.zeros(5)},
              {"labels": torch.zeros(11, 1, dtype=torch.int32)}, {"labels": torch.zeros(12, 1, dtype=torch.int64)},
              {"labels": torch.zeros(12, 33, dtype=torch.int32)}):
    with pytest.raises(ValueError):
      utils.mmd_permutation_test(**dict(ok, **bad))
  for over in ({"general": {"type": "rwpo"}}, {"general": {"type": "ot"}}, {"general": {"type": "fp", "dim": 5}}):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_permutation(solvers.load_config(overrides=over), None, None)
  fpc = solvers.load_config(overrides={"general": {"type": "fp"}})
  for kw in ({"n_particles": 4097}, {"n_particles": 2}, {"times": [0.0, 0.0005]}, {"bandwidths": [1.0] * 9},
             {"n_perm": 254}, {"n_perm": 2047}):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_permutation(fpc, None, None, **kw)
  assert solvers._parse(["--permutation-test"]).permutation_test and not solvers._parse([]).permutation_test
  with pytest.raises(ValueError):      # (the checked-in default is rwpo: refused before any training step)
    solvers.main(solvers.load_config(), permutation_test=True)


@pytest.mark.parametrize("case", P_VALUE_CASES, ids=lambda c: "clouds%d-labels%d" % (c["cloud_seed"], c["label_seed"]))
def test_the_p_value_inputs_keep_every_null_value_away_from_the_observed_one(case):
  x, y, sp, words = p_value_inputs(case)
  member = pr.unpack(words.numpy())
  st = pr.stats(x, y, sp, member)
  floor = 4.0 * EPS * mr.k_max(x, y, sp)
  gap = float(np.abs(st[1:] - st[0]).min())
  p = pr.p_value(st[0], st[1:])
  print(f"[mmd_perm p-value inputs] observed {st[0]:.4e}, min |null - observed| {gap:.2e} against a floor of {floor:.1e}, "
        f"p = {p * len(st):.0f} / {len(st)}")
  assert len(st) == 64 and floor == 4.0 * EPS * 3.0
  assert gap > 4.0 * floor
  assert p == case["p"] and 1.0 / 64.0 < p < 1.0     # (a rank inside the null: the comparison is of a count, not of its floor)
