"""The fused wild-bootstrap test of the kernel Stein discrepancy on the GPU: cnf_stein_boot / utils.ksd_bootstrap_test /
solvers.evaluate_ksd_test, against the float64 restatement (tests/stein_boot_ref.py: q = 2 (S_A + S_B) - t from
stein_ref.stats on the two subsets of every sign vector), with the torch float32 composition on the device -- the Stein
kernel matrix H in float32 from direct differences, its diagonal zeroed, (E * (H E)).sum reduced in float64 -- as the
yardstick:
  e_fused <= 2 e_composed + 4 EPS scale_v,   EPS = 5e-6,
tests/test_gpu_stein.py's bound and derivation for sums[0], applied to EVERY sign vector's statistic: every signed term
is bounded by scale_v (the largest per-pair sum of the absolute values of k_p's four summands), the kernel folds its
float32 accumulators after 64 pair terms, as cnf_stein does, and adds them in double.  t and the diagonal sum are held
to test_gpu_stein.py's bounds for `sum` and `diag`.

The kernel's own boundaries, each with a shape below, at and above it (SHAPES): 16 rows per wave (N = 15, 16, 17),
BOOT_ROWS = 64 rows per workgroup and PAIR_TILE = 64 columns per tile (N = 63, 64, 65; the second tile and row group
fill at N = 128, 129), the column split, which exceeds 1 from the first shape that leaves one tile, N = 65
(cnf_stein_boot_splits, asserted below), and BOOT_CHUNK = 128 sign vectors per pass (P = 128, 160).  The chunk does not
depend on D (every instantiation fits at 128); (8, 70) and (9, 70) stay as the shapes on either side of
the register table's step from three waves per SIMD to two.

Measured on one MI355X (every test prints its figures: run with -s), errors against the restatement, the worst sign
vector of a case, fused / composed:
  the 104 (shape, kernel, P) cases   up to 5.0e-7 / 5.0e-7 (IMQ x 4, D = 1, N = 2: one pair, the pair value's own rounding);
                                     floors 2.3e-5 .. 1.3e-3: at most 0.005 of the floor
  D=10 N=300                         5.5e-9 / 8.7e-9 (Gaussian x 3) .. 2.1e-8 / 1.9e-9 (IMQ x 1)
  D=14 N=129                         3.3e-8 / 9.8e-9 (Gaussian x 1) .. 5.2e-8 / 2.9e-9 (IMQ x 4)
  the chunk boundary, P = 128, 160   2.7e-8 / 1.8e-8 (IMQ x 4), 1.9e-8 / 7.6e-8 (Gaussian x 3)
  t                                  as the values (the worst 5.0e-7 at N = 2); the diagonal sum to 1.6e-15 per point
  vector 0 against t                 0 (the same bits: t is formed as an all +1 vector's q)
  vector 0 against cnf_stein         0 at D = 2, N = 387, both kinds (floors 9.3e-4, 7.0e-4): cnf_stein's lane adds a
                                     tile's 64 columns in the MFMA chain's order
  p-values                           18 / 64 and 25 / 64, the restatement's; values to 6.1e-9
  a cloud shifted by 1.0             KSD^2_U 3.15 (IMQ), 2.67 (Gaussian) over nulls up to 0.70, 0.61: p = 1 / 64
  evaluate_ksd_test, fp / ou         flow 4.7 .. 18.6 at p = 1 / 64 at every time; exact draws 1.0e-2 .. 2.3e-2 at p =
                                     0.0625 (one seed: the same draws, rescaled, at every time); the flow against its own
                                     score -1.4e-3 .. -5.7e-3 at p = 0.50 .. 0.73; the ensemble against the closed-form
                                     score at p = 0.03 .. 0.42; every value equal to evaluate_ksd's in all printed digits
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stein_boot_ref as br
import stein_ref as sr

EPS, P_VALUE_CASES, p_value_inputs = br.EPS, br.P_VALUE_CASES, br.p_value_inputs
BOOT_ROWS, PAIR_TILE, BOOT_CHUNK = 64, 64, 128   # (asserted against the sources below)
# (D, N)
SHAPES = [(1, 2), (2, 15), (2, 16), (2, 17), (2, 63), (2, 64), (2, 65), (3, 128), (3, 129), (8, 70), (9, 70), (14, 129),
          (10, 300)]


def _specs(D):
  r = float(np.sqrt(D))
  return {"imq/1": sr.spec("imq", [r]),
          "imq/4": sr.spec("imq", [0.5 * r, r, 2.0 * r, 4.0 * r], [1.0, 0.5, 0.25, 0.75], beta=-0.75),
          "gaussian/1": sr.spec("gaussian", [r]),
          "gaussian/3": sr.spec("gaussian", [0.5 * r, r, 2.0 * r], [1.0, 0.5, 0.25])}


SPEC_NAMES = list(_specs(1))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, N, index, S=None):
  """(x, s) float32: a Gaussian cloud and a score -A x + b that is not proportional to x"""
  x = sr.cloud(D, N, 7000 + index, scale=1.0 + 0.125 * (index % 5), S=S)
  return x, br.linear_score(x, 8000 + index)


def _signs(N, P, seed=0):
  """(words [N, P / 32] int32 numpy, signs [N, P] bool) of utils.rademacher_signs"""
  from cnf_ot_amd import utils
  words = utils.rademacher_signs(N, P - 1, seed).numpy()
  return words, br.unpack(words)


def _call(dev, x, s, sp, words, want_raw=True, fill=None, stream=None, out=None):
  """cnf_stein_boot through the C ABI on device tensors x, s [S, N, D] and sign words [N, P / 32] (numpy or device
  tensor): (stats [S, P], raw [S (P + 2)] or None, workspace, words on the device).  out: a former result to write into
  (nothing is allocated, nothing waited for)."""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec = utils.stein_spec(**sr.kwargs(sp))
  S, N, D = x.shape
  lib = _capi.lib()
  if out is None:
    wd = torch.from_numpy(np.ascontiguousarray(words)).to(dev) if not torch.is_tensor(words) else words
    P = 32 * wd.shape[1]
    nbytes = ctypes.c_int64(0)
    _capi.check(lib.cnf_stein_boot_workspace(S, N, D, P, ctypes.byref(nbytes)), "cnf_stein_boot_workspace")
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    if fill is not None:
      ws.fill_(fill)
    stats = torch.empty(S, P, dtype=torch.float64, device=dev)
    raw = torch.empty(S * (P + 2), dtype=torch.float64, device=dev) if want_raw else None
  else:
    stats, raw, ws, wd = out
    P = 32 * wd.shape[1]
  assert x.is_contiguous() and s.is_contiguous() and x.dtype == s.dtype == torch.float32 and x.shape == s.shape
  assert wd.is_contiguous() and wd.dtype == torch.int32 and wd.shape[0] == N
  _capi.check(lib.cnf_stein_boot(ctypes.byref(spec), S, x.data_ptr(), s.data_ptr(), N, D, wd.data_ptr(), P, stats.data_ptr(),
                                 None if raw is None else raw.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream_ptr(dev) if stream is None else stream), "cnf_stein_boot")
  if out is None:
    torch.cuda.synchronize()
  return stats, raw, ws, wd


def _qtd(raw, S, P):
  """(q [S, P], t [S], diag [S]) of a raw buffer"""
  return raw[:S * P].view(S, P), raw[S * P:S * (P + 1)], raw[S * (P + 1):]


def _bits(t):
  """A float64 tensor as its bit patterns: NaNs compare equal, -0 and +0 do not"""
  return t.contiguous().view(torch.int64)


def _same(a, b):
  return torch.equal(_bits(a[0]), _bits(b[0])) and (a[1] is None or torch.equal(_bits(a[1]), _bits(b[1])))


def _dev3(dev, a):
  t = torch.from_numpy(a).to(dev)
  return t[None] if t.dim() == 2 else t


def _composed(xd, sd, sp, plus):
  """The torch float32 composition on the device: H in float32 from direct differences, the diagonal zeroed, the signed
  sums in float64; (q [P], t) as float64 numpy / float"""
  D = xd.shape[1]
  d = xd[:, None, :] - xd[None, :, :]
  ds = sd[None, :, :] - sd[:, None, :]
  q = (d * d).sum(-1)
  ss = (sd[:, None, :] * sd[None, :, :]).sum(-1)
  dds = (d * ds).sum(-1)
  p0, p1, p2 = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
  f = np.float32
  for w, bw in zip(sp["w"], sp["bw"]):
    if sp["kind"] == "imq":
      be = sp["beta"]
      u = q + f(bw * bw)
      t = f(w) * u ** f(be)
      p0, p1, p2 = p0 + t, p1 + f(be) * t / u, p2 + f(be * (be - 1.0)) * t / (u * u)
    else:
      ib = 1.0 / (2.0 * bw * bw)
      e = f(w) * torch.exp(-q * f(ib))
      p0, p1, p2 = p0 + e, p1 - f(ib) * e, p2 + f(ib * ib) * e
  H = p0 * ss + f(2.0) * p1 * dds - f(4.0) * p2 * q - f(2.0 * D) * p1
  H.fill_diagonal_(0.0)
  Hd = H.double()
  e = torch.from_numpy(np.where(plus, 1.0, -1.0)).to(Hd.device)
  return (e * (Hd @ e)).sum(0).cpu().numpy(), float(Hd.sum())


@functools.lru_cache(maxsize=None)
def _reference(index, name):
  """(x, s, spec, words [N, 2], signs [N, 64], the restatement) of SHAPES[index]: computed once, shared by the P = 64
  case and the P = 32 case (the first word)"""
  D, N = SHAPES[index]
  x, s = _inputs(D, N, index)
  sp = _specs(D)[name]
  words, plus = _signs(N, 64, seed=index)
  return x, s, sp, words, plus, br.stats(x, s, sp, plus)


WORST = {}


def _check(dev, x, s, sp, words, plus, ref, tag):
  """One set's statistic under every sign vector against the restatement, under the bound above; returns (stats, raw)"""
  N, P = len(x), plus.shape[1]
  pairs = N * (N - 1.0)
  xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev)
  stats, raw, _, _ = _call(dev, xd[None], sd[None], sp, words)
  only, _, _, _ = _call(dev, xd[None], sd[None], sp, words, want_raw=False)
  assert torch.equal(_bits(stats), _bits(only))            # the value does not depend on whether raw is asked for
  got = stats[0].cpu().numpy()
  cq, ct = _composed(xd, sd, sp, plus)
  want = ref["stats"][:P]
  assert np.isfinite(got).all()
  e_fused, e_comp = np.abs(got - want), np.abs(cq / pairs - want)
  floor = 4.0 * EPS * ref["scale_v"]
  worst = int(np.argmax(e_fused - 2.0 * e_comp))
  print(f"\n[stein_boot {tag}] {P} vectors, |value| up to {np.abs(want).max():.3e}: fused up to {e_fused.max():.2e}, "
        f"composed up to {e_comp.max():.2e}, floor {floor:.2e}; the worst vector: fused {e_fused[worst]:.2e} composed "
        f"{e_comp[worst]:.2e}")
  WORST[tag] = (float(e_fused.max()), float(e_comp.max()), floor)
  assert (e_fused <= 2.0 * e_comp + floor).all(), (tag, e_fused[worst], e_comp[worst], floor)
  # raw is what stats is formed from
  q, t, diag = (v.cpu().numpy() for v in _qtd(raw, 1, P))
  assert np.allclose(q[0] / pairs, got, rtol=0.0, atol=1e-13 * max(1.0, ref["scale_v"]))
  # t and the diagonal sum under test_gpu_stein.py's bounds for `sum` and `diag`
  e_t, e_ct = abs(float(t[0]) - ref["t"]) / pairs, abs(ct - ref["t"]) / pairs
  e_d = abs(float(diag[0]) - ref["diag"]) / N
  print(f"[stein_boot {tag}] t: fused {e_t:.2e} composed {e_ct:.2e}; diag: {e_d:.2e} against {4 * EPS * abs(ref['diag']) / N:.2e}")
  assert e_t <= 2.0 * e_ct + floor and e_d <= 4.0 * EPS * abs(ref["diag"]) / N
  return stats, raw


@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("name", SPEC_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-N%d" % s)
def test_every_sign_vector_against_the_restatement(dev, shape, name, P):
  D, N = shape
  x, s, sp, words, plus, ref = _reference(SHAPES.index(shape), name)
  _check(dev, x, s, sp, words[:, :P // 32], plus[:, :P], ref, f"{name} D={D} N={N} P={P}")
  print("[stein_boot] the worst case so far: fused {:.2e} / composed {:.2e} (floor {:.2e})".format(
    *max(WORST.values(), key=lambda v: v[0] / v[2])))


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_stein_boot_splits(1, 64, 2) == 1 and lib.cnf_stein_boot_splits(1, 65, 2) == 2
  assert lib.cnf_stein_boot_splits(1, 128, 3) == 2 and lib.cnf_stein_boot_splits(1, 129, 3) == 3
  assert lib.cnf_stein_boot_splits(1, 300, 10) == 5 and lib.cnf_stein_boot_splits(1, 70, 8) == lib.cnf_stein_boot_splits(1, 70, 9) == 2
  assert lib.cnf_stein_boot_splits(9, 8192, 2) == 2 and lib.cnf_stein_boot_splits(1, 32768, 10) == 4
  csrc = os.path.join(os.path.dirname(_capi.__file__), "csrc")
  src = open(os.path.join(csrc, "cnf_stein_boot.hip")).read()
  assert f"BOOT_CHUNK = {BOOT_CHUNK};" in src and "BOOT_ROWS = 16 * BOOT_WAVES;" in src and "BOOT_THREADS / 64;" in src
  assert f"BOOT_ROWS == {BOOT_ROWS}" in src and "BOOT_TILE = PAIR_TILE" in src
  pairs = open(os.path.join(csrc, "cnf_pairs.h")).read()
  assert re.search(rf"PAIR_TILE = {PAIR_TILE};", pairs) and "PAIR_THREADS = 256;" in pairs


@pytest.mark.parametrize("name", ["imq/4", "gaussian/3"])
@pytest.mark.parametrize("P", [BOOT_CHUNK, BOOT_CHUNK + 32])
def test_the_chunk_boundary(dev, P, name):
  D, N = 2, 70
  x, s = _inputs(D, N, 30)
  sp = _specs(D)[name]
  words, plus = _signs(N, P, seed=30)
  ref = br.stats(x, s, sp, plus)
  # every vector is held to the bound: the last of a pass (BOOT_CHUNK - 1), the first of the next (BOOT_CHUNK), P - 1
  stats, _ = _check(dev, x, s, sp, words, plus, ref, f"chunk {name} P={P}")
  assert stats.shape == (1, P) and not torch.isnan(stats).any()


@pytest.mark.parametrize("name", ["imq/4", "gaussian/3"])
def test_q_does_not_depend_on_P_or_on_the_position(dev, name):
  D, N = 3, 263
  x, s = _inputs(D, N, 31)
  sp = _specs(D)[name]
  xd, sd = _dev3(dev, x), _dev3(dev, s)
  _, plus = _signs(N, 160, seed=31)
  big = _call(dev, xd, sd, sp, br.pack(plus))
  q_big, t_big, d_big = _qtd(big[1], 1, 160)
  # the same vectors elsewhere, among other vectors, in calls of P = 32 and P = 64: across words, blocks and passes
  for P, picks in ((32, [37, 0, 159, 5, 128, 127, 63, 64] + list(range(100, 124))),
                   (64, list(range(159, 95, -1)))):
    small = _call(dev, xd, sd, sp, br.pack(plus[:, picks]))
    q, t, d = _qtd(small[1], 1, P)
    assert torch.equal(_bits(q[0]), _bits(q_big[0, picks]))
    assert torch.equal(_bits(t), _bits(t_big)) and torch.equal(_bits(d), _bits(d_big))
    assert torch.equal(_bits(small[0][0]), _bits(big[0][0, picks]))
  # vector 0 (all +1) is t: the kernel forms t in the chains, the fold and the reduction of an all +1 vector
  scale = sr.stats(x, s, sp)["scale_v"]
  print(f"\n[stein_boot vector 0 against t {name}] {abs(float(q_big[0, 0]) - float(t_big[0])):.2e}")
  assert plus[:, 0].all() and abs(float(q_big[0, 0]) - float(t_big[0])) <= 1e-13 * scale * N * (N - 1.0)


@pytest.mark.parametrize("name", ["imq/4", "gaussian/3"])
def test_the_complement_of_a_sign_vector(dev, name):
  D, N = 2, 341
  x, s = _inputs(D, N, 32)
  sp = _specs(D)[name]
  _, plus = _signs(N, 32, seed=32)
  both = np.concatenate([plus, ~plus], axis=1)            # vector 32 + p: every sign of vector p flipped
  stats, raw, _, _ = _call(dev, _dev3(dev, x), _dev3(dev, s), sp, br.pack(both))
  q, _, _ = _qtd(raw, 1, 64)
  # an fmaf chain with all signs flipped rounds symmetrically, and the row's sign flips it back: the same q bits
  assert torch.equal(_bits(q[0, :32]), _bits(q[0, 32:])) and torch.equal(_bits(stats[0, :32]), _bits(stats[0, 32:]))
  assert len({float(v) for v in q[0, :32]}) == 32


@pytest.mark.parametrize("name", ["imq/4", "gaussian/3"])
def test_vector_0_against_cnf_stein(dev, name):
  from cnf_ot_amd import utils
  D, N = 2, 387
  x, s = _inputs(D, N, 33)
  sp = _specs(D)[name]
  words, _ = _signs(N, 32, seed=33)
  stats, raw, _, _ = _call(dev, _dev3(dev, x), _dev3(dev, s), sp, words)
  direct = utils.ksd(x, s, **sr.kwargs(sp))
  floor = 4.0 * EPS * sr.stats(x, s, sp)["scale_v"]
  print(f"\n[stein_boot against cnf_stein {name}] {float(stats[0, 0]):.6e} against {float(direct['ksd2'][0]):.6e}: "
        f"{abs(float(stats[0, 0]) - float(direct['ksd2'][0])):.2e} (floor {floor:.2e})")
  assert abs(float(stats[0, 0]) - float(direct["ksd2"][0])) <= 2.0 * floor
  # the diagonal sum is cnf_stein's sums[1], row by row in the same double operations
  _, _, diag = _qtd(raw, 1, 32)
  assert abs(float(diag[0]) - float(direct["sums"][0, 1])) <= 1e-12 * abs(float(diag[0]))


@pytest.mark.parametrize("name", ["imq/4", "gaussian/3"])
def test_three_sets_equal_their_own_calls(dev, name):
  from cnf_ot_amd import _capi
  D, N, S = 2, 387, 3
  x, s = _inputs(D, N, 35, S=S)
  x[1] += 0.25                                           # (the sets differ in law as well as in draw)
  sp = _specs(D)[name]
  words, _ = _signs(N, 64, seed=35)
  # (the split count, on which the order of the partial sums depends, is the same for 1 and 3 sets at this size)
  assert _capi.lib().cnf_stein_boot_splits(1, N, D) == _capi.lib().cnf_stein_boot_splits(S, N, D)
  xd, sd = _dev3(dev, x), _dev3(dev, s)
  stats, raw, _, _ = _call(dev, xd, sd, sp, words)
  q, t, d = _qtd(raw, S, 64)
  for k in range(S):
    one = _call(dev, xd[k:k + 1].contiguous(), sd[k:k + 1].contiguous(), sp, words)
    q1, t1, d1 = _qtd(one[1], 1, 64)
    assert torch.equal(_bits(stats[k]), _bits(one[0][0])) and torch.equal(_bits(q[k]), _bits(q1[0]))
    assert float(t[k]) == float(t1[0]) and float(d[k]) == float(d1[0])
  assert len({round(float(v), 6) for v in stats[:, 0]}) == S      # three different numbers: no set read twice


def test_more_than_64_sets_through_the_python_surface(dev):
  from cnf_ot_amd import utils
  D, N, S = 2, 44, 66
  x, s = _inputs(D, N, 36, S=S)
  sp = _specs(D)["imq/4"]
  kw = sr.kwargs(sp)
  res = utils.ksd_bootstrap_test(x, s, n_boot=31, seed=36, **kw)
  assert set(res) == {"ksd2", "null", "p_value", "ksd2_v", "null_v", "p_value_v", "raw", "bandwidths"}
  assert set(res["raw"]) == {"q", "t", "diag"}
  assert res["ksd2"].shape == (S,) and res["null"].shape == (S, 31) and res["p_value"].shape == (S,)
  assert res["ksd2_v"].shape == (S,) and res["null_v"].shape == (S, 31) and res["p_value_v"].shape == (S,)
  assert res["raw"]["q"].shape == (S, 32) and res["raw"]["t"].shape == (S,) and res["raw"]["diag"].shape == (S,)
  assert all(res[k].dtype == torch.float64 for k in ("ksd2", "null", "p_value", "ksd2_v", "null_v", "p_value_v"))
  assert res["bandwidths"] == sp["bw"]
  for k in (0, 63, 64, 65):                              # both calls: a set equals its own call bit for bit
    one = utils.ksd_bootstrap_test(x[k], s[k], n_boot=31, seed=36, **kw)
    assert one["ksd2"].shape == (1,) and torch.equal(_bits(one["ksd2"]), _bits(res["ksd2"][k:k + 1]))
    assert torch.equal(_bits(one["null"][0]), _bits(res["null"][k])) and float(one["p_value"][0]) == float(res["p_value"][k])
    assert torch.equal(_bits(one["null_v"][0]), _bits(res["null_v"][k]))
    assert float(one["raw"]["t"][0]) == float(res["raw"]["t"][k]) and float(one["raw"]["diag"][0]) == float(res["raw"]["diag"][k])
  assert torch.equal(res["p_value"], utils.permutation_p_value(res["ksd2"], res["null"]))
  assert torch.equal(res["ksd2_v"], (res["raw"]["q"][:, 0] + res["raw"]["diag"]) / (float(N) * N))


def test_two_calls_a_dirty_workspace_and_a_captured_graph_give_the_same_bits(dev):
  for (D, N, S), name, P in (((3, 1200, 2), "imq/4", 64), ((14, 129, 1), "gaussian/3", 160)):
    x, s = _inputs(D, N, 37, S=S)
    sp = _specs(D)[name]
    words, _ = _signs(N, P, seed=37)
    xd, sd = _dev3(dev, x), _dev3(dev, s)
    first = _call(dev, xd, sd, sp, words)
    assert _same(first, _call(dev, xd, sd, sp, words))
    assert _same(first, _call(dev, xd, sd, sp, words, fill=0xFF))      # (0xFF bytes: NaN doubles wherever not rewritten)
    # one call replayed from a captured graph (a single stream: no parallel branches)
    out = (torch.zeros_like(first[0]), torch.zeros_like(first[1]), torch.full_like(first[2], 0xFF), first[3])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph, stream=side):
        _call(dev, xd, sd, sp, words, stream=side.cuda_stream, out=out)
      graph.replay()
    side.synchronize()
    assert _same(first, out)


def test_refusals_leave_the_outputs_untouched(dev):
  from cnf_ot_amd import _capi, utils
  D, N, P = 2, 70, 64
  x, s = _inputs(D, N, 38)
  xd, sd = _dev3(dev, x), _dev3(dev, s)
  words, _ = _signs(N, P, seed=38)
  wd = torch.from_numpy(words).to(dev)
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_stein_boot_workspace(1, N, D, P, ctypes.byref(nbytes)), "cnf_stein_boot_workspace")
  ws = torch.full((nbytes.value,), 0x5A, dtype=torch.uint8, device=dev)
  stats = torch.full((P,), 7.0, dtype=torch.float64, device=dev)
  raw = torch.full((P + 2,), 7.0, dtype=torch.float64, device=dev)

  def spec(**kw):
    sp = utils.stein_spec("imq", [1.0, 2.0])
    for k, v in kw.items():
      if isinstance(v, tuple):
        getattr(sp, k)[v[0]] = v[1]
      else:
        setattr(sp, k, v)
    return sp

  good = dict(spec=spec(), S=1, x=xd.data_ptr(), score=sd.data_ptr(), N=N, D=D, signs=wd.data_ptr(), P=P,
              stats=stats.data_ptr(), raw=raw.data_ptr(), ws=ws.data_ptr(), wsb=nbytes.value)

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
              {"spec": spec(kind=2, bw=(0, 1e-7))}, {"wsb": nbytes.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad
  torch.cuda.synchronize()
  assert bool((stats == 7.0).all()) and bool((raw == 7.0).all()) and bool((ws == 0x5A).all())
  assert call() == _capi.CNF_OK                          # ... and the good call writes all of stats and raw
  torch.cuda.synchronize()
  assert not bool((stats == 7.0).any()) and not bool((raw == 7.0).any())


@pytest.mark.parametrize("case", P_VALUE_CASES, ids=lambda c: "cloud%d-signs%d" % (c["cloud_seed"], c["sign_seed"]))
def test_p_values_equal_the_restatements(dev, case):
  from cnf_ot_amd import utils
  x, s, sp, words = p_value_inputs(case)                 # (their gap condition: tests/test_stein_boot_cpu.py)
  ref = br.stats(x, s, sp, br.unpack(words.numpy()))["stats"]
  want = br.p_value(ref[0], ref[1:])
  res = utils.ksd_bootstrap_test(x, s, n_boot=case["n_boot"], seed=case["sign_seed"], **sr.kwargs(sp))
  print(f"\n[stein_boot p-value] {float(res['p_value'][0]) * 64:.0f} / 64 against {want * 64:.0f} / 64; values to "
        f"{float(np.abs(torch.cat([res['ksd2'], res['null'][0]]).cpu().numpy() - ref).max()):.2e}")
  assert float(res["p_value"][0]) == want == case["p"]
  # the signs given are the signs drawn
  own = utils.ksd_bootstrap_test(x, s, signs=words, **sr.kwargs(sp))
  assert torch.equal(_bits(own["null"]), _bits(res["null"])) and torch.equal(own["p_value"], res["p_value"])


@pytest.mark.parametrize("kind", ["imq", "gaussian"])
def test_a_shifted_cloud_gets_the_smallest_p_value(dev, kind):
  from cnf_ot_amd import utils
  x = (sr.cloud(2, 96, 5) + np.float32(1.0)).astype(np.float32)      # N(1, I) against the score of N(0, I)
  res = utils.ksd_bootstrap_test(x, -x, kind=kind, n_boot=63)         # (the default bandwidths: the median heuristic)
  print(f"\n[stein_boot shifted {kind}] ksd2 {float(res['ksd2'][0]):.4e}, null up to {float(res['null'].max()):.4e}")
  assert float(res["p_value"][0]) == 1.0 / 64.0 and float(res["ksd2"][0]) > float(res["null"].max())
  assert float(res["p_value_v"][0]) == 1.0 / 64.0 and len(res["bandwidths"]) == 4


def test_evaluate_ksd_test(dev):
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  n, seed, n_boot = 1024, 5, 63
  res = solvers.evaluate_ksd_test(config, model, params, n=n, seed=seed, n_boot=n_boot)
  rows = solvers.KSD_TEST_ROWS
  assert rows == ("flow", "floor", "ensemble", "ensemble_flow", "flow_own")
  assert set(res) == {"times", "kind", "n", "n_boot"} | set(rows) | {"p_" + k for k in rows}
  assert res["n"] == n and res["n_boot"] == n_boot and res["kind"] == "imq" and len(res["times"]) >= 2
  assert all(len(res[k]) == len(res["p_" + k]) == len(res["times"]) for k in rows)
  solvers.print_ksd_test(res)
  # a flow with random parameters is told apart from the target at the smallest level 64 vectors can state ...
  assert res["p_flow"] == [1.0 / 64.0] * len(res["times"])
  # ... and where the null holds -- exact draws against their own score, the flow's samples against the flow's score --
  # the p-values are uniform, so each exceeds 0.01 in 99 of 100 draws.  A condition on this fixed seed: should another
  # seed miss it, confirm with the restatement on the same points (br.stats) that the reference misses it too before
  # changing the seed.
  for k in ("p_floor", "p_flow_own"):
    assert all(p > 0.01 for p in res[k]), (k, res[k])
  # the values are evaluate_ksd's at the same arguments: the same sets, scores and bandwidths through the other kernel
  base = solvers.evaluate_ksd(config, model, params, n=n, seed=seed)
  assert base["times"] == res["times"]
  entries = app.known_densities(config)
  f = config["fp"]
  pos = app.fp_reference_particles(2, f["T"], f["a"], f["sigma"], f["velocity_field_type"], res["times"], n, 1e-3, seed,
                                   positions=True)["pos"].float()
  from cnf_ot_amd import utils
  for i, (t, target, scale) in enumerate(entries):
    x = model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n,)).float()
    exact = solvers.target_draws(target, scale, n, seed).to(dev)
    sets = {"flow": (x, target.score(x, scale), exact), "floor": (exact, target.score(exact, scale), exact),
            "ensemble": (pos[i], target.score(pos[i], scale), pos[i]),
            "ensemble_flow": (pos[i], model.apply.score(params, pos[i].contiguous(), cond=float(t)), pos[i]),
            "flow_own": (x, model.apply.score(params, x.contiguous(), cond=float(t)), pos[i])}
    for k, (pts, score, bw_of) in sets.items():
      sp = sr.spec("imq", utils.median_bandwidths(bw_of)[:4])
      floor = 4.0 * EPS * sr.stats(pts.cpu().numpy(), score.float().cpu().numpy(), sp)["scale_v"]
      print(f"[evaluate_ksd_test {k} t={t}] {res[k][i]:+.6e} against {base[k][i]:+.6e} (floor {floor:.2e})")
      assert abs(res[k][i] - base[k][i]) <= 2.0 * floor, (k, i)
  # another type: no ensemble columns
  ot = solvers.evaluate_ksd_test(solvers.load_config(overrides={"general": {"type": "ot", "dim": 2}}), model, params, n=n,
                                 seed=seed, n_boot=31)
  assert ot["ensemble"] is None and ot["p_flow_own"] is None and len(ot["flow"]) == len(ot["p_floor"]) == len(ot["times"]) == 2
  solvers.print_ksd_test(ot)
