"""The fused permutation test of the kernel two-sample statistics on the GPU: cnf_mmd_perm / utils.mmd_permutation_test /
solvers.evaluate_fp_permutation, against the float64 restatement (tests/mmd_perm_ref.py: mmd_ref.mmd2 on the two subsets
of every label vector), with the torch float32 composition on the device -- the pooled kernel matrix K in float32 from
direct differences, its diagonal zeroed, the signed sums q, r, t reduced in float64 -- as the yardstick:
  e_fused <= 2 e_composed + 4 eps k_max,   eps = 5e-6,
tests/test_gpu_mmd.py's bound and derivation, applied to EVERY label vector's statistic: the kernel folds its float32
accumulators after 64 pair terms, as cnf_mmd2 does, and the signed terms are bounded by k_max.

The kernel's own boundaries, each with a shape below, at and above it (SHAPES): 16 rows per wave (n = N + M = 15, 16,
17), PERM_ROWS = 64 rows per workgroup and PAIR_TILE = 64 columns per tile (n = 63, 64, 65; the second tile and row
group fill at n = 128, 129), the column split, which exceeds 1 from the first shape whose pooled sample leaves one
tile, n = 65 (cnf_mmd_perm_splits, asserted below), and PERM_CHUNK = 128 label vectors per pass (P = 128, 160).

Measured on one MI355X (every test prints its figures: run with -s), errors against the restatement, the worst label
vector of a case, fused / composed:
  the 96 (shape, kernel, P) cases   up to 5.6e-7 / 7.9e-8 (Gaussian x 8, N = 33, M = 32) and, at N = M = 2, 3.8e-7 /
                                    2.8e-7; floors 2e-5 .. 2.8e-4: at most 0.006 of the floor
  D=10 N=300 M=257                  8.5e-10 / 1.2e-9 (Gaussian x 1) .. 3.4e-8 / 3.0e-9 (energy)
  D=14 N=129 M=64                   2.1e-9 / 5.7e-10 (Gaussian x 1) .. 2.0e-7 / 2.1e-8 (Gaussian x 8)
  the chunk boundary, P = 128, 160  2.6e-8 / 8.6e-9 (Gaussian x 3), 3.7e-8 / 9.4e-9 (energy)
  counts of their own               1.4e-5 / 6.9e-8 (Gaussian x 3), 5.7e-5 / 2.3e-8 (energy), both at the vector with
                                    N_p = 2 of n = 161: 0.2 and 0.4 of the floor (the identity's cancellation, DESIGN.md
                                    5.3t); the other vectors 2.7e-8 / 5.0e-9 and 3.5e-8 / 7.7e-9
  vector 0 against cnf_mmd2         3.6e-8 (Gaussian x 3, floor 6e-5), 2.1e-9 (energy, floor 1.8e-4)
  p-values                          3 / 64 and 28 / 64, the restatement's; values to 3.2e-8
  evaluate_fp_permutation, ou       mmd2 0.68, 0.72 and energy 0.89, 0.91 at p = 1 / 64; halves 5.8e-4 (p 0.375), 4.5e-3
                                    (0.0625) and 1.9e-4 (0.359), 2.0e-3 (0.219) (random parameters, 1 024 particles)
"""
import ctypes
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_perm_ref as pr
import mmd_ref as mr

EPS, P_VALUE_CASES, p_value_inputs = pr.EPS, pr.P_VALUE_CASES, pr.p_value_inputs
PERM_ROWS, PAIR_TILE, PERM_CHUNK = 64, 64, 128   # (asserted against the sources below)
# (D, N, M)
SHAPES = [(1, 2, 2), (2, 7, 8), (2, 8, 8), (2, 8, 9), (2, 31, 32), (2, 32, 32), (2, 33, 32), (3, 64, 64), (3, 64, 65),
          (14, 129, 64), (10, 300, 257), (2, 257, 130)]
KERNELS = [("gaussian", 1), ("gaussian", 3), ("gaussian", 8), ("energy", 0)]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _spec(kind, D, n_bw):
  # the bandwidths as the kernel receives them (float32)
  return mr.spec(kind, [float(np.float32(math.sqrt(D) * 0.5 * 2.0 ** b)) for b in range(n_bw)] if kind == "gaussian" else ())


def _inputs(D, N, M, index, S=None):
  return mr.clouds(D, N, M, seed=2000 + index, shift=0.2 + 0.1 * (index % 4), scale=1.0 + 0.125 * (index % 5), S=S)


def _labels(N, M, P, seed=0):
  """(words [n, P / 32] int32 numpy, membership [n, P]) of utils.permutation_labels"""
  from cnf_ot_amd import utils
  words = utils.permutation_labels(N, M, P - 1, seed).numpy()
  return words, pr.unpack(words)


def _call(dev, x, y, sp, words, want_raw=True, fill=None, stream=None, out=None):
  """cnf_mmd_perm through the C ABI on device tensors x [S, N, D], y [S, M, D] and label words [n, P / 32] (numpy or
  device tensor): (stats [S, P], raw [S (2 P + 1)] or None, workspace, words on the device).  out: a former result to
  write into (nothing is allocated, nothing waited for)."""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec, _ = utils.mmd_spec(sp["bw"], sp["kind"])
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  if out is None:
    wd = torch.from_numpy(np.ascontiguousarray(words)).to(dev) if not torch.is_tensor(words) else words
    P = 32 * wd.shape[1]
    nbytes = ctypes.c_int64(0)
    _capi.check(lib.cnf_mmd_perm_workspace(S, N, M, D, P, ctypes.byref(nbytes)), "cnf_mmd_perm_workspace")
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    if fill is not None:
      ws.fill_(fill)
    stats = torch.empty(S, P, dtype=torch.float64, device=dev)
    raw = torch.empty(S * (2 * P + 1), dtype=torch.float64, device=dev) if want_raw else None
  else:
    stats, raw, ws, wd = out
    P = 32 * wd.shape[1]
  assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.float32
  assert wd.is_contiguous() and wd.dtype == torch.int32 and wd.shape[0] == N + M
  _capi.check(lib.cnf_mmd_perm(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, wd.data_ptr(), P, stats.data_ptr(),
                               None if raw is None else raw.data_ptr(), ws.data_ptr(), ws.numel(),
                               _stream_ptr(dev) if stream is None else stream), "cnf_mmd_perm")
  if out is None:
    torch.cuda.synchronize()
  return stats, raw, ws, wd


def _qrt(raw, S, P):
  """(q [S, P], r [S, P], t [S]) of a raw buffer"""
  qr = raw[:S * 2 * P].view(S, P, 2)
  return qr[..., 0], qr[..., 1], raw[S * 2 * P:]


def _bits(t):
  """A float64 tensor as its bit patterns: NaNs compare equal, -0 and +0 do not"""
  return t.contiguous().view(torch.int64)


def _same(a, b):
  return torch.equal(_bits(a[0]), _bits(b[0])) and (a[1] is None or torch.equal(_bits(a[1]), _bits(b[1])))


def _dev3(dev, a):
  t = torch.from_numpy(a).to(dev)
  return t[None] if t.dim() == 2 else t


def _composed(xd, yd, sp, member):
  """The torch float32 composition on the device: K of the pooled sample in float32 from direct differences, the
  diagonal zeroed, the signed sums in float64; the statistic per label vector [P] as float64 numpy"""
  z = torch.cat([xd, yd])
  diff = z[:, None, :] - z[None, :, :]
  d2 = (diff * diff).sum(-1)
  if sp["kind"] == "energy":
    k = -torch.sqrt(d2)
  else:
    k = torch.zeros_like(d2)
    for bw in sp["bw"]:
      k = k + torch.exp(-d2 / np.float32(2.0 * bw * bw))
  k.fill_diagonal_(0.0)
  kd = k.double()
  s = torch.from_numpy(np.where(member, 1.0, -1.0)).to(kd.device)
  ks = kd @ s
  q, r, t = (s * ks).sum(0).cpu().numpy(), ks.sum(0).cpu().numpy(), float(kd.sum())
  return pr.stats_of_qrt(q, r, t, member.sum(0), len(z))


@functools.lru_cache(maxsize=None)
def _reference(index, kind, n_bw):
  """(x, y, spec, words [n, 2], membership [n, 64], the restatement's statistic [64]) of SHAPES[index]: computed once,
  shared by the P = 64 case and the P = 32 case (the first word)"""
  D, N, M = SHAPES[index]
  x, y = _inputs(D, N, M, index)
  sp = _spec(kind, D, n_bw)
  words, member = _labels(N, M, 64, seed=index)
  return x, y, sp, words, member, pr.stats(x, y, sp, member)


def _check(dev, x, y, sp, words, member, ref, tag):
  """One set's statistic under every label vector against the restatement, under the bound above; returns the stats"""
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  stats, raw, _, _ = _call(dev, xd[None], yd[None], sp, words)
  only, _, _, _ = _call(dev, xd[None], yd[None], sp, words, want_raw=False)
  assert torch.equal(_bits(stats), _bits(only))            # the value does not depend on whether raw is asked for
  got = stats[0].cpu().numpy()
  comp = _composed(xd, yd, sp, member)
  ok = ~np.isnan(ref)
  assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(np.isnan(comp), ~ok)
  e_fused, e_comp = np.abs(got - ref)[ok], np.abs(comp - ref)[ok]
  floor = 4.0 * EPS * mr.k_max(x, y, sp)
  worst = int(np.argmax(e_fused - 2.0 * e_comp))
  print(f"\n[mmd_perm {tag}] {ok.sum()} vectors, |value| up to {np.abs(ref[ok]).max():.3e}: fused up to {e_fused.max():.2e}, "
        f"composed up to {e_comp.max():.2e}, floor {floor:.2e}; the worst vector: fused {e_fused[worst]:.2e} composed "
        f"{e_comp[worst]:.2e}")
  assert (e_fused <= 2.0 * e_comp + floor).all(), (tag, e_fused[worst], e_comp[worst], floor)
  # raw is what stats is formed from
  q, r, t = (v.cpu().numpy() for v in _qrt(raw, 1, member.shape[1]))
  again = pr.stats_of_qrt(q[0], r[0], t[0], member.sum(0), len(x) + len(y))
  assert np.allclose(again[ok], got[ok], rtol=0.0, atol=1e-13 * max(1.0, mr.k_max(x, y, sp)))
  return stats


@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("kind,n_bw", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-N%d-M%d" % s)
def test_every_label_vector_against_the_restatement(dev, shape, kind, n_bw, P):
  D, N, M = shape
  x, y, sp, words, member, ref = _reference(SHAPES.index(shape), kind, n_bw)
  _check(dev, x, y, sp, words[:, :P // 32], member[:, :P], ref[:P], f"{kind}/{n_bw} D={D} N={N} M={M} P={P}")


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_mmd_perm_splits(1, 32, 32, 2) == 1 and lib.cnf_mmd_perm_splits(1, 33, 32, 2) == 2    # n = 64 -> 65
  assert lib.cnf_mmd_perm_splits(1, 64, 64, 3) == 2 and lib.cnf_mmd_perm_splits(1, 64, 65, 3) == 3
  assert lib.cnf_mmd_perm_splits(1, 300, 257, 10) == 9 and lib.cnf_mmd_perm_splits(3, 257, 130, 2) == 7
  assert lib.cnf_mmd_perm_splits(9, 4096, 4096, 2) == 2 and lib.cnf_mmd_perm_splits(1, 32768, 32768, 10) == 2
  csrc = os.path.join(os.path.dirname(_capi.__file__), "csrc")
  src = open(os.path.join(csrc, "cnf_mmd_perm.hip")).read()
  assert f"PERM_CHUNK = {PERM_CHUNK};" in src and "PERM_ROWS = 16 * PERM_WAVES;" in src and "PERM_THREADS / 64;" in src
  assert f"PERM_ROWS == {PERM_ROWS}" in src and "PERM_TILE = PAIR_TILE" in src
  pairs = open(os.path.join(csrc, "cnf_pairs.h")).read()
  assert re.search(rf"PAIR_TILE = {PAIR_TILE};", pairs) and "PAIR_THREADS = 256;" in pairs


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
@pytest.mark.parametrize("P", [PERM_CHUNK, PERM_CHUNK + 32])
def test_the_chunk_boundary(dev, P, kind, n_bw):
  D, N, M = 2, 70, 60
  x, y = _inputs(D, N, M, 30)
  sp = _spec(kind, D, n_bw)
  words, member = _labels(N, M, P, seed=30)
  ref = pr.stats(x, y, sp, member)
  # every vector is held to the bound: the last of a pass (PERM_CHUNK - 1), the first of the next (PERM_CHUNK), P - 1
  stats = _check(dev, x, y, sp, words, member, ref, f"chunk {kind}/{n_bw} P={P}")
  assert stats.shape == (1, P) and not torch.isnan(stats).any()


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
def test_q_and_r_do_not_depend_on_P_or_on_the_position(dev, kind, n_bw):
  D, N, M = 3, 150, 113
  x, y = _inputs(D, N, M, 31)
  sp = _spec(kind, D, n_bw)
  xd, yd = _dev3(dev, x), _dev3(dev, y)
  _, member = _labels(N, M, 160, seed=31)
  big = _call(dev, xd, yd, sp, pr.pack(member))
  q_big, r_big, t_big = _qrt(big[1], 1, 160)
  # the same vectors elsewhere, among other vectors, in calls of P = 32 and P = 64: across words, blocks and passes
  for P, picks in ((32, [37, 0, 159, 5, 128, 127, 63, 64] + list(range(100, 124))),
                   (64, list(range(159, 95, -1)))):
    small = _call(dev, xd, yd, sp, pr.pack(member[:, picks]))
    q, r, t = _qrt(small[1], 1, P)
    assert torch.equal(_bits(q[0]), _bits(q_big[0, picks])) and torch.equal(_bits(r[0]), _bits(r_big[0, picks]))
    assert torch.equal(_bits(t), _bits(t_big))
    assert torch.equal(_bits(small[0][0]), _bits(big[0][0, picks]))


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 5), ("energy", 0)])
def test_the_complement_of_a_label_vector(dev, kind, n_bw):
  D, N, M = 2, 200, 141
  x, y = _inputs(D, N, M, 32)
  sp = _spec(kind, D, n_bw)
  _, member = _labels(N, M, 32, seed=32)
  both = np.concatenate([member, ~member], axis=1)        # vector 32 + p: every bit of vector p flipped
  stats, raw, _, _ = _call(dev, _dev3(dev, x), _dev3(dev, y), sp, pr.pack(both))
  q, r, _ = _qrt(raw, 1, 64)
  # an fmaf chain with all signs flipped rounds symmetrically: the same q bits, r negated, the same statistic
  assert torch.equal(_bits(q[0, :32]), _bits(q[0, 32:]))
  assert torch.equal(_bits(r[0, :32]), _bits(-r[0, 32:]))
  assert float(r[0].abs().min()) > 0.0
  assert torch.equal(_bits(stats[0, :32]), _bits(stats[0, 32:]))


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
def test_vector_0_against_cnf_mmd2(dev, kind, n_bw):
  from cnf_ot_amd import utils
  D, N, M = 2, 257, 130
  x, y = _inputs(D, N, M, 33)
  sp = _spec(kind, D, n_bw)
  words, _ = _labels(N, M, 32, seed=33)
  stats, _, _, _ = _call(dev, _dev3(dev, x), _dev3(dev, y), sp, words)
  direct = float(utils.mmd2(x, y, sp["bw"] or None, kind)["mmd2"][0])
  floor = 4.0 * EPS * mr.k_max(x, y, sp)
  print(f"\n[mmd_perm against cnf_mmd2 {kind}] {float(stats[0, 0]):.6e} against {direct:.6e}: "
        f"{abs(float(stats[0, 0]) - direct):.2e} (floor {floor:.2e})")
  assert abs(float(stats[0, 0]) - direct) <= 2.0 * floor


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
def test_label_vectors_with_their_own_counts(dev, kind, n_bw):
  D, N, M = 2, 90, 71
  n = N + M
  x, y = _inputs(D, N, M, 34)
  sp = _spec(kind, D, n_bw)
  _, member = _labels(N, M, 64, seed=34)
  member = member.copy()
  member[N:N + 7, 3] = True                              # N_p = N + 7 (vector 3 was some subset: set seven more bits)
  member[:, 3] |= np.arange(n) < 5
  member[:, 9] = np.arange(n) < 2                        # N_p = 2
  member[:, 40] = np.arange(n) >= 2                      # M_p = 2
  member[:, 41] = np.arange(n) % 3 == 0
  ref = pr.stats(x, y, sp, member)
  assert len({int(c) for c in member.sum(0)}) >= 5 and not np.isnan(ref).any()
  base = _check(dev, x, y, sp, pr.pack(member), member, ref, f"counts {kind}/{n_bw}")
  # vectors outside the legal range give NaN for themselves alone: every other vector keeps its bits
  bad = member.copy()
  bad[:, 9] = np.arange(n) == 17                         # one set bit
  bad[:, 40] = np.arange(n) != 17                        # one clear bit
  bad[:, 41] = False                                     # an empty first sample
  bad[:, 63] = True                                      # an empty second sample
  out = _check(dev, x, y, sp, pr.pack(bad), bad, pr.stats(x, y, sp, bad), f"counts, four illegal vectors {kind}/{n_bw}")
  keep = [p for p in range(64) if p not in (9, 40, 41, 63)]
  assert torch.isnan(out[0, [9, 40, 41, 63]]).all() and not torch.isnan(out[0, keep]).any()
  assert torch.equal(_bits(out[0, keep]), _bits(base[0, keep]))


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
def test_three_sets_equal_their_own_calls(dev, kind, n_bw):
  from cnf_ot_amd import _capi
  D, N, M, S = 2, 257, 130, 3
  x, y = _inputs(D, N, M, 35, S=S)
  y[1] += 0.25                                           # (the sets differ in law as well as in draw)
  sp = _spec(kind, D, n_bw)
  words, _ = _labels(N, M, 64, seed=35)
  # (the split count, on which the order of the partial sums depends, is the same for 1 and 3 sets at this size)
  assert _capi.lib().cnf_mmd_perm_splits(1, N, M, D) == _capi.lib().cnf_mmd_perm_splits(S, N, M, D)
  xd, yd = _dev3(dev, x), _dev3(dev, y)
  stats, raw, _, _ = _call(dev, xd, yd, sp, words)
  q, r, t = _qrt(raw, S, 64)
  for s in range(S):
    one = _call(dev, xd[s:s + 1].contiguous(), yd[s:s + 1].contiguous(), sp, words)
    q1, r1, t1 = _qrt(one[1], 1, 64)
    assert torch.equal(_bits(stats[s]), _bits(one[0][0]))
    assert torch.equal(_bits(q[s]), _bits(q1[0])) and torch.equal(_bits(r[s]), _bits(r1[0])) and float(t[s]) == float(t1[0])
  assert len({round(float(v), 6) for v in stats[:, 0]}) == S      # three different numbers: no set read twice


def test_more_than_64_sets_through_the_python_surface(dev):
  from cnf_ot_amd import utils
  D, N, M, S = 2, 20, 24, 66
  x, y = _inputs(D, N, M, 36, S=S)
  bws = _spec("gaussian", D, 2)["bw"]
  res = utils.mmd_permutation_test(x, y, bws, n_perm=31, seed=36)
  assert set(res) == {"mmd2", "null", "p_value", "counts", "bandwidths", "raw"} and set(res["raw"]) == {"q", "r", "t"}
  assert res["mmd2"].shape == (S,) and res["null"].shape == (S, 31) and res["p_value"].shape == (S,)
  assert res["raw"]["q"].shape == (S, 32) and res["raw"]["r"].shape == (S, 32) and res["raw"]["t"].shape == (S,)
  assert res["mmd2"].dtype == torch.float64 and res["counts"].tolist() == [N] * 32 and res["bandwidths"] == bws
  for s in (0, 63, 64, 65):                              # both calls: a set equals its own call bit for bit
    one = utils.mmd_permutation_test(x[s], y[s], bws, n_perm=31, seed=36)
    assert one["mmd2"].shape == (1,) and torch.equal(_bits(one["mmd2"]), _bits(res["mmd2"][s:s + 1]))
    assert torch.equal(_bits(one["null"][0]), _bits(res["null"][s])) and float(one["p_value"][0]) == float(res["p_value"][s])
    assert float(one["raw"]["t"][0]) == float(res["raw"]["t"][s])
  assert torch.equal(res["p_value"], utils.permutation_p_value(res["mmd2"], res["null"]))


def test_two_calls_a_dirty_workspace_and_a_captured_graph_give_the_same_bits(dev):
  for (D, N, M, S), (kind, n_bw), P in (((3, 700, 500, 2), ("gaussian", 5), 64), ((14, 129, 64, 1), ("energy", 0), 160)):
    x, y = _inputs(D, N, M, 37, S=S)
    sp = _spec(kind, D, n_bw)
    words, _ = _labels(N, M, P, seed=37)
    xd, yd = _dev3(dev, x), _dev3(dev, y)
    first = _call(dev, xd, yd, sp, words)
    assert _same(first, _call(dev, xd, yd, sp, words))
    assert _same(first, _call(dev, xd, yd, sp, words, fill=0xFF))      # (0xFF bytes: NaN doubles wherever not rewritten)
    # one call replayed from a captured graph (a single stream: no parallel branches)
    out = (torch.zeros_like(first[0]), torch.zeros_like(first[1]), torch.full_like(first[2], 0xFF), first[3])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph, stream=side):
        _call(dev, xd, yd, sp, words, stream=side.cuda_stream, out=out)
      graph.replay()
    side.synchronize()
    assert _same(first, out)


def test_refusals_leave_the_outputs_untouched(dev):
  from cnf_ot_amd import _capi
  D, N, M, P = 2, 40, 30, 64
  x, y = _inputs(D, N, M, 38)
  xd, yd = _dev3(dev, x), _dev3(dev, y)
  words, _ = _labels(N, M, P, seed=38)
  wd = torch.from_numpy(words).to(dev)
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_perm_workspace(1, N, M, D, P, ctypes.byref(nbytes)), "cnf_mmd_perm_workspace")
  ws = torch.full((nbytes.value,), 0x5A, dtype=torch.uint8, device=dev)
  stats = torch.full((P,), 7.0, dtype=torch.float64, device=dev)
  raw = torch.full((2 * P + 1,), 7.0, dtype=torch.float64, device=dev)

  def spec(kind=0, bws=(1.0, 2.0)):
    s = _capi.CnfMmdSpec()
    s.kind, s.n_bw = kind, len(bws)
    for i, b in enumerate(bws[:8]):
      s.bw[i] = b
    return s

  good = dict(spec=spec(), S=1, x=xd.data_ptr(), N=N, y=yd.data_ptr(), M=M, D=D, labels=wd.data_ptr(), P=P,
              stats=stats.data_ptr(), raw=raw.data_ptr(), ws=ws.data_ptr(), wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_mmd_perm(None if a["spec"] is None else ctypes.byref(a["spec"]), a["S"], a["x"], a["N"], a["y"], a["M"],
                            a["D"], a["labels"], a["P"], a["stats"], a["raw"], a["ws"], a["wsb"], None)

  for bad in ({"spec": None}, {"x": None}, {"y": None}, {"labels": None}, {"stats": None}, {"ws": None}, {"D": 0}, {"D": 15},
              {"N": 1}, {"M": 1}, {"S": 0}, {"S": 65}, {"N": (1 << 20) - M + 1}, {"P": 0}, {"P": 16}, {"P": 48}, {"P": 1056},
              {"spec": spec(kind=2)}, {"spec": spec(bws=())}, {"spec": spec(bws=(1.0,) * 9)}, {"spec": spec(bws=(1.0, 0.0))},
              {"spec": spec(bws=(float("nan"),))}, {"spec": spec(bws=(1e-30,))}, {"wsb": nbytes.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad
  torch.cuda.synchronize()
  assert bool((stats == 7.0).all()) and bool((raw == 7.0).all()) and bool((ws == 0x5A).all())
  assert call() == _capi.CNF_OK                          # ... and the good call writes all of stats and raw
  torch.cuda.synchronize()
  assert not bool((stats == 7.0).any()) and not bool((raw == 7.0).any())


@pytest.mark.parametrize("case", P_VALUE_CASES, ids=lambda c: "clouds%d-labels%d" % (c["cloud_seed"], c["label_seed"]))
def test_p_values_equal_the_restatements(dev, case):
  from cnf_ot_amd import utils
  x, y, sp, words = p_value_inputs(case)                 # (their gap condition: tests/test_mmd_perm_cpu.py)
  ref = pr.stats(x, y, sp, pr.unpack(words.numpy()))
  want = pr.p_value(ref[0], ref[1:])
  res = utils.mmd_permutation_test(x, y, sp["bw"], n_perm=case["n_perm"], seed=case["label_seed"])
  print(f"\n[mmd_perm p-value] {float(res['p_value'][0]) * 64:.0f} / 64 against {want * 64:.0f} / 64; values to "
        f"{float(np.abs(torch.cat([res['mmd2'], res['null'][0]]).cpu().numpy() - ref).max()):.2e}")
  assert float(res["p_value"][0]) == want == case["p"]
  # the labels given are the labels drawn
  own = utils.mmd_permutation_test(x, y, sp["bw"], labels=words)
  assert torch.equal(_bits(own["null"]), _bits(res["null"])) and torch.equal(own["p_value"], res["p_value"])


@pytest.mark.parametrize("kind", ["gaussian", "energy"])
def test_shifted_clouds_get_the_smallest_p_value(dev, kind):
  from cnf_ot_amd import utils
  x, y = mr.clouds(2, 96, 80, seed=5, shift=2.0, scale=1.0)
  res = utils.mmd_permutation_test(x, y, kind=kind, n_perm=63)      # (the default bandwidths: the median heuristic)
  assert float(res["p_value"][0]) == 1.0 / 64.0 and float(res["mmd2"][0]) > float(res["null"].max())
  assert len(res["bandwidths"]) == (5 if kind == "gaussian" else 0)


def test_evaluate_fp_permutation(dev):
  from cnf_ot_amd import FlowConfig, Params, solvers, utils
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  n, h, seed, n_perm, times = 1024, 1e-2, 5, 63, [0.0, 0.1]
  res = solvers.evaluate_fp_permutation(config, model, params, times=times, n_particles=n, h=h, seed=seed, n_perm=n_perm)
  keys = [p + k + t for k in ("mmd2", "energy") for t in ("", "_halves") for p in ("", "p_")]
  assert set(res) == set(keys) | {"times", "bandwidths", "n_perm"} and res["times"] == times and res["n_perm"] == n_perm
  solvers.print_fp_permutation(res)
  # a flow with random parameters is told apart from the ensemble at the smallest level 64 vectors can state ...
  assert res["p_mmd2"] == [1.0 / 64.0] * 2 and res["p_energy"] == [1.0 / 64.0] * 2
  # ... and the two halves, two samples of one law, are not: their p-values are uniform, so each exceeds 0.01 in 99 of
  # 100 draws.  A condition on this fixed seed: should another seed miss it, confirm with the restatement on the same
  # positions (pr.stats on the halves) that the reference misses it too before changing the seed.
  for k in ("p_mmd2_halves", "p_energy_halves"):
    assert all(p > 0.01 for p in res[k]), (k, res[k])
  # the table's numbers are utils.mmd_permutation_test's on the same samples, labels and bandwidths
  _, ts, _, fp = solvers._fp_prelude("test", config, times, n, h, 4)
  flow, h0, h1 = solvers._fp_flow_and_halves(model, params, fp, ts, n, h, seed)
  labels = utils.permutation_labels(n // 2, n // 2, n_perm, seed)
  bws = utils.median_bandwidths(h0)
  assert res["bandwidths"] == [float(np.float32(b)) for b in bws]
  for kind, key in (("gaussian", "mmd2"), ("energy", "energy")):
    for first, tail in ((flow, ""), (h1, "_halves")):
      want = utils.mmd_permutation_test(first, h0, bws, kind, labels=labels)
      assert res[key + tail] == want["mmd2"].tolist() and res["p_" + key + tail] == want["p_value"].tolist()
