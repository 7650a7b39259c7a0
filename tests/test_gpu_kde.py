"""The fused kernel density estimate on the GPU: cnf_kde / utils.kde / applications.ensemble_fields /
solvers.evaluate_fp_fields, against the float64 restatement (tests/kde_ref.py), with the same composition in float32 --
t and exp(t - m) in float32, reduced in float64 -- as the yardstick of the fused error, the project's bar
(test_gpu_interaction.py, test_gpu_stein.py), per query i and coordinate d:
  e_fused <= 2 e_composed + 4 EPS scale,   EPS = 5e-6
  scale(log_rho)  = 1 + |m_i|                                     (m_i = max_j t_ij: float32 carries t to 2^-24 |t|)
  scale(score_d)  = (1 + |m_i|) sum_j w_ij |x_jd - q_id| / h^2    (the weights carry exp's argument, the sum its terms)
  sums: the bar of log_rho on sums / Q, with the mean of the rows' scales
The kernel's float32 sums live for one tile of 64 columns (64 * 2^-24 = 3.8e-6 of the tile's sum at the very worst); the
pair's rounding (differences, the fmaf chain of d2, one subtraction, one multiplication, v_exp_f32) is a few 2^-24 of |t|.

The kernel's own boundaries, each with a shape below, at and above it: the 64-column tile (N = 63, 64, 65); the rows of
one workgroup, 256 lanes x rows per lane -- two where n_bw (1 + D) <= 16 (Q = 511, 512, 513), one above ((D, n_bw) =
(10, 4), (14, 4): Q = 255, 256, 257); more than one row group AND more than one split (asserted below).  Q != N in
every query-mode case.  Bandwidths: sqrt(D) / 2 times (1) or (0.5, 1, 2, 4).

Every test prints its figures (run with -s); the worst share of the bar measured on one MI355X is in DESIGN.md 5.3r.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kde_ref as kr

EPS = 5e-6
FACTOR = 0.5
# (D, n_bw, N, Q)
CASES = [(2, 1, 63, 37), (2, 1, 64, 37), (2, 1, 65, 37), (2, 4, 63, 37), (2, 4, 64, 37), (2, 4, 65, 37),
         (3, 1, 130, 511), (3, 1, 130, 512), (3, 1, 130, 513), (2, 4, 130, 511), (2, 4, 130, 512), (2, 4, 130, 513),
         (10, 4, 70, 255), (10, 4, 70, 256), (10, 4, 70, 257), (14, 4, 70, 255), (14, 4, 70, 257),
         (1, 1, 700, 600), (1, 4, 300, 1030), (3, 4, 300, 1030), (10, 1, 200, 520), (14, 1, 200, 520), (14, 4, 200, 520),
         (10, 4, 1, 5), (3, 1, 2, 3)]
MULTI = [(1, 1, 700, 600), (1, 4, 300, 1030), (3, 4, 300, 1030), (10, 1, 200, 520), (14, 1, 200, 520), (14, 4, 200, 520)]


def _rows(D, B):
  return 256 * (2 if B * (1 + D) <= 16 else 1)


def _bws(D, B):
  r = FACTOR * float(np.sqrt(D))
  return kr.bandwidths([r] if B == 1 else [0.5 * r, r, 2.0 * r, 4.0 * r])


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, N, Q, index, scale=1.0, shift=0.0):
  """(x [N, D], q [Q, D]) float32: a Gaussian cloud and queries 1.5 times as wide, so that tails are among them"""
  return kr.cloud(D, N, 7000 + index, scale, shift), kr.cloud(D, Q, 8000 + index, 1.5 * scale, shift)


@functools.lru_cache(maxsize=None)
def _reference(D, B, N, Q, index, self_mode=False, loo=False):
  """Per bandwidth, the restatement of one case and its float32 composition, computed once"""
  x, q = _inputs(D, N, Q, index)
  q = None if self_mode else q
  return [(kr.kde(x, q, h, loo), kr.kde(x, q, h, loo, dtype=np.float32)) for h in _bws(D, B)]


def _call(dev, x, q, bws, loo=False, want=(True, True, True), fill=None, stream=None, out=None):
  """cnf_kde through the C ABI on device tensors x [S, N, D], q [S, Q, D] or None: (log_rho [S, B, Q] or None, score
  [S, B, Q, D] or None, sums [S, B] or None, workspace).  out: a former result to write into (nothing is allocated,
  nothing waited for)."""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec = utils.kde_spec(bws, loo)
  S, N, D = x.shape
  Q, B = N if q is None else q.shape[1], len(bws)
  lib = _capi.lib()
  need = ctypes.c_int64(0)
  _capi.check(lib.cnf_kde_workspace(S, N, Q, D, B, int(want[1]), ctypes.byref(need)), "cnf_kde_workspace")
  if out is None:
    ws = torch.zeros(need.value, dtype=torch.uint8, device=dev)
    if fill is not None:
      ws.fill_(fill)
    lr = torch.empty(S, B, Q, dtype=torch.float32, device=dev) if want[0] else None
    sc = torch.empty(S, B, Q, D, dtype=torch.float32, device=dev) if want[1] else None
    sums = torch.empty(S, B, dtype=torch.float64, device=dev) if want[2] else None
  else:
    lr, sc, sums, ws = out
  assert x.is_contiguous() and x.dtype == torch.float32 and (q is None or (q.is_contiguous() and q.dtype == torch.float32))
  ptr = lambda t: None if t is None else t.data_ptr()
  _capi.check(lib.cnf_kde(ctypes.byref(spec), S, x.data_ptr(), N, ptr(q), Q, D, ptr(lr), ptr(sc), ptr(sums), ws.data_ptr(),
                          need.value, _stream_ptr(dev) if stream is None else stream), "cnf_kde")
  if out is None:
    torch.cuda.synchronize()
  return lr, sc, sums, ws


def _same(a, b):
  return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a[:3], b[:3]))


SHARES = {}


def _check(lr, sc, total, ref, comp, tag):
  """One (set, bandwidth): log_rho [Q], score [Q, D] and the sum against the restatement under the bar above"""
  n64 = lambda t: t.cpu().double().numpy()
  lr, sc = n64(lr), n64(sc)
  Q = len(lr)
  s_lr = 1.0 + np.abs(ref["m"])
  s_sc = s_lr[:, None] * ref["absw"]
  e = {"log_rho": (np.abs(lr - ref["log_rho"]), np.abs(comp["log_rho"] - ref["log_rho"]), s_lr),
       "score": (np.abs(sc - ref["score"]), np.abs(comp["score"] - ref["score"]), s_sc),
       "sums": (np.abs(float(total) / Q - ref["log_rho"].mean()), np.abs(comp["log_rho"].mean() - ref["log_rho"].mean()),
                s_lr.mean())}
  print(f"\n[kde {tag}] mean log_rho {ref['log_rho'].mean():+.5f} | " + " | ".join(
    f"{k}: fused {np.max(a):.2e} composed {np.max(b):.2e} floor {4 * EPS * np.max(c):.2e}" for k, (a, b, c) in e.items()))
  assert np.isfinite(lr).all() and np.isfinite(sc).all() and np.isfinite(float(total))
  for k, (a, b, c) in e.items():
    bar = 2.0 * b + 4.0 * EPS * c
    share = float(np.max(np.where(bar > 0.0, a / np.where(bar > 0.0, bar, 1.0), 0.0)))
    SHARES[k] = max(SHARES.get(k, 0.0), share)
    assert (a <= bar).all(), (tag, k, float(np.max(a - bar)), share)


def _dev3(dev, a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)[None].contiguous()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "D%d-B%d-N%d-Q%d" % c)
def test_log_density_score_and_sums_against_the_restatement(dev, case):
  D, B, N, Q = case
  index = CASES.index(case)
  x, q = _inputs(D, N, Q, index)
  bws = _bws(D, B)
  got = _call(dev, _dev3(dev, x), _dev3(dev, q), bws)
  # no output depends on which others are asked for
  for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
    other = _call(dev, _dev3(dev, x), _dev3(dev, q), bws, want=want)
    assert all(o is None or torch.equal(o, g) for o, g in zip(other[:3], got[:3])), want
  for b, (ref, comp) in enumerate(_reference(D, B, N, Q, index)):
    _check(got[0][0, b], got[1][0, b], got[2][0, b], ref, comp, f"D={D} B={B} N={N} Q={Q} h={bws[b]:.4g}")
  print("[kde] worst shares of the bar so far: " + " ".join(f"{k} {v:.3f}" for k, v in SHARES.items()))


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_kde_splits(1, 64, 37, 2) == 1 and lib.cnf_kde_splits(1, 65, 37, 2) == 2
  for D, B, N, Q in MULTI:                       # more than one row group and more than one split
    assert -(-Q // _rows(D, B)) >= 2 and lib.cnf_kde_splits(1, N, Q, D) > 1
  assert lib.cnf_kde_splits(3, 200, 520, 3) > 1
  assert lib.cnf_kde_splits(0, 8, 8, 2) < 0 and lib.cnf_kde_splits(1, 8, 8, 15) < 0 and lib.cnf_kde_splits(1, 0, 8, 2) < 0
  src = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "cnf_kde.hip")).read()
  assert "KD_THREADS = 256;" in src and "KD_TILE = 64;" in src and "return NB * (1 + D) <= 16 ? 2 : 1;" in src
  # the workspace grows with the score and with the bandwidths
  size = lambda B, score: _ws_bytes(lib, 2, 300, 520, 3, B, score)
  assert size(1, 0) < size(1, 1) < size(4, 1) and size(1, 0) < size(4, 0)


def _ws_bytes(lib, S, N, Q, D, B, score):
  n = ctypes.c_int64(0)
  assert lib.cnf_kde_workspace(S, N, Q, D, B, score, ctypes.byref(n)) == 0
  return n.value


def test_the_c_abi_refuses_before_any_launch(dev):
  from cnf_ot_amd import _capi, utils
  lib = _capi.lib()
  x = torch.zeros(1, 8, 2, device=dev)
  q = torch.zeros(1, 5, 2, device=dev)
  lr = torch.full((1, 2, 8), 7.0, device=dev)
  sc = torch.full((1, 2, 8, 2), 7.0, device=dev)
  sums = torch.full((1, 2), 7.0, dtype=torch.float64, device=dev)
  ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
  P = lambda t: t.data_ptr()

  def rc(spec, S=1, xp=P(x), N=8, qp=None, Q=8, D=2, lrp=P(lr), scp=P(sc), sp=P(sums), wsp=P(ws), nbytes=1 << 16):
    return lib.cnf_kde(ctypes.byref(spec) if spec is not None else None, S, xp, N, qp, Q, D, lrp, scp, sp, wsp, nbytes, None)
  good = utils.kde_spec([1.0, 2.0])

  def bad(**kw):
    sp = utils.kde_spec([1.0, 2.0])
    for k, v in kw.items():
      if isinstance(v, tuple):
        getattr(sp, k)[v[0]] = v[1]
      else:
        setattr(sp, k, v)
    return sp
  inf, nan = float("inf"), float("nan")
  for sp in (bad(n_bw=0), bad(n_bw=5), bad(bw=(1, 0.0)), bad(bw=(0, -1.0)), bad(bw=(0, inf)), bad(bw=(1, nan)),
             bad(bw=(0, 1e-20)), bad(bw=(1, 1e20)), None):
    assert rc(sp) == _capi.CNF_ERR_INVALID
  for kw in (dict(S=0), dict(S=65), dict(N=0, Q=0), dict(N=(1 << 20) + 1, Q=(1 << 20) + 1), dict(D=0), dict(D=15),
             dict(Q=5),                                           # self mode with Q != N
             dict(qp=P(q), Q=0), dict(qp=P(q), Q=(1 << 20) + 1), dict(xp=None), dict(wsp=None),
             dict(lrp=None, scp=None, sp=None), dict(nbytes=8)):
    assert rc(good, **kw) == _capi.CNF_ERR_INVALID, kw
  assert rc(bad(loo=1), qp=P(q), Q=5) == _capi.CNF_ERR_INVALID      # leave-one-out with queries of their own
  assert rc(bad(loo=1), N=1, Q=1) == _capi.CNF_ERR_INVALID
  nb = ctypes.c_int64(-1)
  for args in ((0, 8, 8, 2, 1, 1), (1, 0, 8, 2, 1, 1), (1, 8, 0, 2, 1, 1), (1, 8, 8, 15, 1, 1), (1, 8, 8, 2, 0, 1),
               (1, 8, 8, 2, 5, 1)):
    assert lib.cnf_kde_workspace(*args, ctypes.byref(nb)) == _capi.CNF_ERR_INVALID and nb.value == -1
  assert lib.cnf_kde_workspace(1, 8, 8, 2, 1, 1, None) == _capi.CNF_ERR_INVALID
  torch.cuda.synchronize()
  assert float(sums[0, 0]) == 7.0 and bool((lr == 7.0).all()) and bool((sc == 7.0).all())      # nothing was enqueued
  assert rc(good) == _capi.CNF_OK and rc(bad(loo=1)) == _capi.CNF_OK and rc(good, N=1, Q=1) == _capi.CNF_OK
  torch.cuda.synchronize()
  assert float(sums[0, 0]) != 7.0


@pytest.mark.parametrize("shape", [(2, 1, 513), (3, 4, 300), (10, 4, 257), (14, 1, 130)], ids=lambda s: "D%d-B%d-N%d" % s)
def test_self_mode_with_and_without_leave_one_out(dev, shape):
  D, B, N = shape
  index = 100 + D
  x, _ = _inputs(D, N, 1, index)
  bws = _bws(D, B)
  xd = _dev3(dev, x)
  full, loo = _call(dev, xd, None, bws), _call(dev, xd, None, bws, loo=True)
  as_query = _call(dev, xd, xd.clone(), bws)
  assert _same(full, as_query)                    # self mode without loo is the query mode on the same points
  refs_full, refs_loo = _reference(D, B, N, 1, index, True, False), _reference(D, B, N, 1, index, True, True)
  for b, h in enumerate(bws):
    _check(full[0][0, b], full[1][0, b], full[2][0, b], *refs_full[b], f"self D={D} B={B} N={N} h={h:.4g}")
    _check(loo[0][0, b], loo[1][0, b], loo[2][0, b], *refs_loo[b], f"loo D={D} B={B} N={N} h={h:.4g}")
    # the leave-one-out identity from the call without it: rho_loo = (N rho - (2 pi h^2)^(-D / 2)) / (N - 1)
    lf, ll = full[0][0, b].cpu().double().numpy(), loo[0][0, b].cpu().double().numpy()
    own = -0.5 * D * np.log(2.0 * np.pi * h * h)
    rho_n = N * np.exp(lf - own) - 1.0            # (in units of the own term: the other points' share, >= 0)
    want = own + np.log(np.maximum(rho_n, 1e-300)) - np.log(N - 1.0)
    # where the own term dominates, the difference cancels: the bar is log_rho's on N rho, divided by what is left
    tol = 4.0 * (2.0 * EPS * (1.0 + np.abs(refs_full[b][0]["m"]))) * (rho_n + 1.0) / np.maximum(rho_n, 1e-300) + 4.0 * EPS * (
      1.0 + np.abs(refs_loo[b][0]["m"]))
    ok = rho_n > 1e-3
    print(f"[kde loo identity D={D} h={h:.4g}] rows checked {int(ok.sum())}/{N}, worst {np.abs(ll - want)[ok].max():.2e}")
    assert ok.sum() >= N // 4 and (np.abs(ll - want)[ok] <= tol[ok]).all()


def test_three_sets_of_different_scale(dev):
  D, B, N, Q = 3, 4, 150, 530
  scales = (1.0, 0.05, 30.0)
  xs, qs = zip(*[_inputs(D, N, Q, 200 + k, scale=s, shift=s * k) for k, s in enumerate(scales)])
  bws = kr.bandwidths([0.05, 0.5, 2.0, 20.0])
  xd = torch.from_numpy(np.stack(xs)).to(dev)
  qd = torch.from_numpy(np.stack(qs)).to(dev)
  got = _call(dev, xd, qd, bws)
  for k in range(3):
    alone = _call(dev, xd[k:k + 1].contiguous(), qd[k:k + 1].contiguous(), bws)
    assert torch.equal(alone[0][0], got[0][k]) and torch.equal(alone[1][0], got[1][k])
    for b, h in enumerate(bws):
      lr = got[0][k, b].cpu().double().numpy()
      ref, comp = kr.kde(xs[k], qs[k], h), kr.kde(xs[k], qs[k], h, dtype=np.float32)
      live = np.isfinite(comp["log_rho"])          # (scale 30 with h = 0.05: some rows have no source within reach)
      if live.all():
        _check(got[0][k, b], got[1][k, b], got[2][k, b], ref, comp, f"set {k} scale {scales[k]} h={h:.4g}")
      else:
        assert (np.isneginf(lr) == ~live).all(), (k, h)


def test_far_queries_out_of_reach_and_duplicates(dev):
  D, N = 2, 200
  x, _ = _inputs(D, N, 1, 300)
  x[10] = x[3]
  x[11] = x[3]                                     # duplicated points
  h = 1.0
  q = np.concatenate([x[:5], np.array([[1000.0, 0.0], [-700.0, 700.0], [1e25, 0.0], [0.0, -1e25], [3.0, 3.0]], np.float32)])
  got = _call(dev, _dev3(dev, x), _dev3(dev, q), [h])
  lr, sc = got[0][0, 0].cpu().numpy(), got[1][0, 0].cpu().numpy()
  ref, comp = kr.kde(x, q, h), kr.kde(x, q, h, dtype=np.float32)
  assert abs(ref["m"][5] + 5e5) < 2e4              # t about -5e5
  keep = [0, 1, 2, 3, 4, 5, 6, 9]
  sub = lambda r: {k: v[keep] for k, v in r.items()}
  assert np.isfinite(lr[keep]).all()
  _check(torch.from_numpy(lr[keep]), torch.from_numpy(sc[keep]), float(lr[keep].astype(np.float64).sum()), sub(ref), sub(comp),
         "far queries and duplicates")
  assert np.isneginf(lr[7]) and np.isneginf(lr[8]) and (sc[7] == 0.0).all() and (sc[8] == 0.0).all()
  # leave-one-out: the copies of point 3 at other indices still count
  loo = _call(dev, _dev3(dev, x), None, [h], loo=True)
  rl, cl = kr.kde(x, None, h, loo=True), kr.kde(x, None, h, loo=True, dtype=np.float32)
  _check(loo[0][0, 0], loo[1][0, 0], loo[2][0, 0], rl, cl, "duplicates, leave-one-out")
  own = -np.log(2.0 * np.pi * h * h) - np.log(N - 1.0)
  assert float(loo[0][0, 0, 3]) >= own + np.log(2.0) - 1e-4


def test_nan_stays_where_the_contract_says(dev):
  D, B, N, Q, S = 3, 4, 130, 520, 3
  bws = _bws(D, B)
  xs = np.stack([_inputs(D, N, Q, 400 + k)[0] for k in range(S)])
  qs = np.stack([_inputs(D, N, Q, 400 + k)[1] for k in range(S)])
  clean = _call(dev, torch.from_numpy(xs).to(dev), torch.from_numpy(qs).to(dev), bws)
  assert all(bool(torch.isfinite(t).all()) for t in clean[:3])
  # one query
  qn = qs.copy()
  qn[1, 300, 2] = np.nan
  got = _call(dev, torch.from_numpy(xs).to(dev), torch.from_numpy(qn).to(dev), bws)
  hit = torch.zeros(S, B, Q, dtype=torch.bool, device=dev)
  hit[1, :, 300] = True
  assert bool(torch.isnan(got[0][hit]).all()) and bool(torch.isnan(got[1][hit]).all())
  assert torch.equal(got[0][~hit], clean[0][~hit]) and torch.equal(got[1][~hit], clean[1][~hit])
  assert bool(torch.isnan(got[2][1]).all()) and torch.equal(got[2][[0, 2]], clean[2][[0, 2]])
  # one source of one set
  xn = xs.copy()
  xn[2, 77, 0] = np.nan
  got = _call(dev, torch.from_numpy(xn).to(dev), torch.from_numpy(qs).to(dev), bws)
  assert bool(torch.isnan(got[0][2]).all()) and bool(torch.isnan(got[1][2]).all()) and bool(torch.isnan(got[2][2]).all())
  for t, c in zip(got[:3], clean[:3]):
    assert torch.equal(t[:2], c[:2])
  # self mode with leave-one-out: the set is NaN, the others are not touched
  xl = torch.from_numpy(xs).to(dev)
  clean_loo = _call(dev, xl, None, bws, loo=True)
  got = _call(dev, torch.from_numpy(xn).to(dev), None, bws, loo=True)
  assert bool(torch.isnan(got[0][2]).all()) and torch.equal(got[0][:2], clean_loo[0][:2]) and torch.equal(got[1][:2], clean_loo[1][:2])


def test_two_calls_a_dirty_workspace_and_a_captured_graph_give_the_same_bits(dev):
  for D, B, N, Q, loo in ((3, 4, 300, 1030, False), (14, 4, 200, 520, False), (2, 1, 700, 700, True)):
    x, q = _inputs(D, N, Q, 500 + D)
    xd, qd = _dev3(dev, x), (None if loo else _dev3(dev, q))
    bws = _bws(D, B)
    first = _call(dev, xd, qd, bws, loo=loo)
    assert _same(first, _call(dev, xd, qd, bws, loo=loo))
    assert _same(first, _call(dev, xd, qd, bws, loo=loo, fill=0xFF))
    # one call replayed from a captured graph
    out = tuple(torch.zeros_like(t) for t in first[:3]) + (torch.full_like(first[3], 0xFF),)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph, stream=side):
        _call(dev, xd, qd, bws, loo=loo, stream=side.cuda_stream, out=out)
      graph.replay()
    side.synchronize()
    assert _same(first, out)


def test_utils_kde_is_the_c_abi_call(dev):
  from cnf_ot_amd import utils
  D, N, Q = 3, 300, 530
  x, q = _inputs(D, N, Q, 600)
  bws = _bws(D, 4)
  xd, qd = _dev3(dev, x), _dev3(dev, q)
  raw = _call(dev, xd, qd, bws)
  res = utils.kde(qd, xd, bws)
  assert torch.equal(res["log_density"], raw[0]) and torch.equal(res["score"], raw[1])
  assert torch.equal(res["mean_log_density"], raw[2] / Q) and res["mean_log_density"].dtype == torch.float64
  assert res["bandwidths"] == bws
  # [N, D] inputs drop the axis; host and float64 inputs are staged
  flat = utils.kde(torch.from_numpy(q).double(), x, bws, want_score=False)
  assert flat["score"] is None and flat["log_density"].shape == (4, Q) and torch.equal(flat["log_density"], raw[0][0])
  assert flat["mean_log_density"].shape == (4,) and flat["log_density"].is_cuda
  # self mode: leave-one-out by default
  raw_loo, raw_self = _call(dev, xd, None, bws, loo=True), _call(dev, xd, None, bws)
  own = utils.kde(x, bandwidths=bws)
  assert torch.equal(own["log_density"], raw_loo[0][0]) and torch.equal(own["score"], raw_loo[1][0])
  assert torch.equal(utils.kde(xd, bandwidths=bws, loo=False)["log_density"], raw_self[0])
  # bandwidths=None: the normal-reference rule of the sources
  auto = utils.kde(qd, xd)
  h = utils.kde_bandwidths(xd)
  assert auto["bandwidths"] == kr.bandwidths(h) and torch.equal(auto["log_density"], _call(dev, xd, qd, kr.bandwidths(h))[0])
  # the leave-one-out likelihood picks a bandwidth of the rule's order for a Gaussian cloud
  like = utils.kde(xd, bandwidths=[0.05 * h[0], h[0], 20.0 * h[0]])["mean_log_density"][0]
  assert float(like[1]) > float(like[0]) and float(like[1]) > float(like[2])
  for kw in (dict(points=qd, sources=xd, loo=True), dict(points=qd, sources=xd[:, :, :2]), dict(points=qd, sources=xd, bandwidths=[0.0])):
    with pytest.raises(ValueError):
      utils.kde(**kw)


def test_ensemble_fields_is_its_composition(dev):
  from cnf_ot_amd import applications as app, utils
  for sub, D, kw, strength in (("ou", 3, None, 0.0), ("gradient", 2, None, 0.0), ("nongradient", 2, None, 0.0),
                               ("lorenz", 3, None, 0.0),
                               ("ou", 2, dict(kind="gaussian", amplitudes=[1.0], bandwidths=[0.7]), 0.4),
                               ("ou", 2, dict(kind="quadratic"), 0.25)):
    x, q = _inputs(D, 400, 300, 700 + D)
    xd, qd = torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev)
    bws = _bws(D, 4)[:2]
    sigma, a = 0.5, 0.75
    got = app.ensemble_fields(qd, xd, sigma, a, sub, bws, kw, strength)
    est = utils.kde(qd, xd, bws)
    vel = app.fp_drift(qd, a, sub)[None] - sigma * est["score"]
    if kw is not None:
      vel = vel - strength * utils.interaction_field(qd, xd, **kw)["force"][None]
    assert torch.equal(got["log_density"], est["log_density"]) and torch.equal(got["score"], est["score"])
    assert got["velocity"].shape == (2, 300, D) and torch.equal(got["velocity"], vel) and got["bandwidths"] == est["bandwidths"]
    # several sets keep their axis
    both = app.ensemble_fields(torch.stack([qd, qd]), torch.stack([xd, xd]), sigma, a, sub, bws, kw, strength)
    assert both["velocity"].shape == (2, 2, 300, D) and torch.equal(both["velocity"][1], got["velocity"])
  with pytest.raises(ValueError):
    app.ensemble_fields(qd, xd, 0.5, 1.0, "lorenz", [1.0])
  with pytest.raises(ValueError):
    app.ensemble_fields(qd, xd, float("nan"), 1.0, "ou", [1.0])


def _fp_config(interaction=None):
  from cnf_ot_amd import solvers
  over = {"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}}
  if interaction is not None:
    over["interaction"] = interaction
  return solvers.load_config(None, over)


@pytest.mark.parametrize("interacting", [False, True], ids=["free", "interacting"])
def test_evaluate_fp_fields_is_its_recomputation_from_the_public_pieces(dev, interacting):
  from cnf_ot_amd import applications as app, solvers, utils
  from cnf_ot_amd.distributed import Shard
  config = _fp_config({"kind": "quadratic", "role": "drift"} if interacting else None)
  model = solvers.build_model(config)
  params = model.init(0)                     # the untrained flow: the identity
  times, n_particles, n_points, h, seed = [0.25, 0.5], 4096, 256, 1e-3, 3
  res = solvers.evaluate_fp_fields(config, model, params, times, n_particles, n_points, h, seed, bandwidth_factor=1.5)
  solvers.print_fp_fields(res)
  keys = [k for k in solvers.FP_FIELD_KEYS[:8]] + ([] if interacting else ["kde_score_bias"])
  assert res["times"] == times and res["n"] == 2048 and res["n_points"] == 256
  assert (res["kde_score_bias"] is None) == interacting
  for k in keys:
    assert len(res[k]) == 2 and np.isfinite(res[k]).all(), k
  f, g = config["fp"], config["general"]
  dim, T, a, sigma, sub = g["dim"], f["T"], f["a"], f["sigma"], f["velocity_field_type"]
  if interacting:
    kw, strength = solvers._interaction_kwargs(config), float(config["interaction"]["strength"])
    pos = app.mv_reference_particles(dim, T, a, sigma, sub, kw, strength, times, 2048, 2, h, seed, positions=True)["pos"]
    h0, h1 = pos[:, 0].float(), pos[:, 1].float()
  else:
    kw, strength = None, 0.0
    h0, h1 = (app.fp_reference_particles(dim, T, a, sigma, sub, times, n_particles, h, seed, positions=True,
                                         shard=Shard(r, 2), all_reduce=False)["pos"].float() for r in (0, 1))
  rel = lambda u, v: float(((u.double() - v.double()) ** 2).sum() / (v.double() ** 2).sum())
  for i, t in enumerate(times):
    src, pts = h0[i].contiguous(), h1[i, :n_points].contiguous()
    bw = 1.5 * utils.kde_bandwidths(src)[0]
    assert res["bandwidth"][i] == float(np.float32(bw))
    est = utils.kde(pts, src, [bw])
    vel = app.fp_drift(pts, a, sub) - sigma * est["score"][0]
    if interacting:
      vel = vel - strength * utils.interaction_field(pts, src, **kw)["force"]
    flow = utils.eulerian_fields(model, params, pts, [t], logp=True, vel=True, score=True, exact_score=True, dt=g["dt"])
    assert res["logp_rmse"][i] == float(((flow["logp"][0].double() - est["log_density"][0].double()) ** 2).mean().sqrt())
    assert res["score_rel_err"][i] == rel(flow["score"][0], est["score"][0])
    assert res["velocity_rel_err"][i] == rel(flow["vel"][0], vel)
    ha, hb = utils.kde(pts, src[:1024].contiguous(), [bw]), utils.kde(pts, src[1024:].contiguous(), [bw])
    assert res["logp_rmse_floor"][i] == float(((ha["log_density"][0].double() - hb["log_density"][0].double()) ** 2).mean().sqrt())
    assert res["score_rel_err_floor"][i] == rel(ha["score"][0], hb["score"][0])
    if not interacting:
      exact = pts.double() * (-1.0 / app.ou_variance(t, a, app.fp_initial_variance(T), sigma))
      assert res["kde_score_bias"][i] == rel(est["score"][0], exact)
      # the estimate is an estimate of the law: its score is the closed form's up to the bandwidth's bias and the noise
      assert res["kde_score_bias"][i] < 0.25 and res["score_rel_err_floor"][i] < 0.25


def test_evaluate_fp_fields_and_the_flag_refuse_before_any_work():
  from cnf_ot_amd import solvers
  config = _fp_config()
  for kw in (dict(n_particles=6), dict(n_particles=4098), dict(n_points=0), dict(n_points=3000, n_particles=4096),
             dict(bandwidth_factor=0.0), dict(bandwidth_factor=float("nan")), dict(times=[0.00015])):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_fields(config, None, None, **kw)
  ot = solvers.load_config(None, {"general": {"type": "ot"}})
  with pytest.raises(ValueError):
    solvers.evaluate_fp_fields(ot, None, None)
  with pytest.raises(ValueError, match="--field-errors"):
    solvers.main(ot, epochs=0, field_errors=True)
  assert solvers._parse(["--field-errors"]).field_errors and not solvers._parse([]).field_errors
