"""The fused nearest-neighbour scan on the GPU: cnf_knn / utils.knn / utils.knn_divergence / solvers.evaluate_fp_knn,
against the float64 restatement (tests/knn_ref.py).

Exact-grid clouds (coordinates that are multiples of 1/8 in [-4, 4]: every d2 is exact in float32, ties and duplicates
are plentiful): dist, idx and the zero counts equal the restatement BIT FOR BIT, the log sums to 1e-10 per mean.
Gaussian clouds: every distance within (D + 4) 2^-24 relative of the restatement's (one rounding per difference, three
per square-and-add, the square root halves it; the k-th order statistic is 1-Lipschitz in the sup norm), the log means
within the same bound plus 1e-12, and the index wherever the restatement's gap to both neighbouring ranks exceeds
twice that bound (at most 1 % of the entries are left out: tests/test_knn_cpu.py pins that).

The kernel's own constants, each with a shape below, at and above it (EXACT_SHAPES; asserted against cnf_knn_splits and
the source in test_the_boundaries_named_above_are_the_kernels): KNN_ROWS = 512 rows per workgroup (N = 511, 512, 513 --
at 513 the diagonal of the second workgroup's row lies in its own tile, and the first workgroup's rows meet the
diagonal in tiles of its own only), KNN_TILE = 64 columns per tile, the unit the split is counted in (M = 63, 64, 65),
the first shape with 2 splits (max(N, M) = 65; at N = 65, M = 64 the cross block's second split is EMPTY and at M = 65
it holds one column, fewer than k), N = k + 1 with M = k (every other point is a neighbour), k = 1, the compiled
capacities 4 and 16, and 5 = the small capacity plus 1 (17 is refused: tests/test_knn_cpu.py), D in {1, 2, 3, 10, 14}.

Measured on one MI355X (every test prints its figures: run with -s), against the restatement:
  Gaussian clouds, 4 shapes x k = 4, 16   distances 9.6e-8 .. 1.5e-7 relative (bounds 3.6e-7 .. 1.07e-6), log means
                                          1.3e-9 .. 9.1e-9, indices compared 0.9990 .. 1.0000 of the entries, all equal
  knn_divergence                          2.6e-9 .. 6.0e-9 nats at D = 2 (bound 7.2e-7), 1.8e-8 .. 4.0e-8 at D = 10 (8.3e-6)
  identity flow against N(0, 2 I)         kl 0.165 (closed form 0.193), kl_floor -0.012, entropies 2.8526 (kNN) and
                                          2.8523 (model) against 2.838; kl_reverse 0.158 against 0.307 (the estimator's
                                          bias where the cloud searched is the narrower one; the restatement agrees),
                                          kl_ensemble_flow 0.303
More cases: profiles/knn/README.md.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as kr

# (D, N, M, k)
EXACT_SHAPES = [(2, 511, 63, 4), (2, 512, 64, 4), (2, 513, 65, 4), (3, 64, 64, 4), (3, 65, 64, 4), (1, 5, 4, 4), (1, 17, 16, 16),
                (2, 130, 65, 16), (10, 300, 257, 5), (14, 129, 64, 16), (2, 1025, 1024, 1), (3, 700, 1100, 16), (1, 600, 70, 5)]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _call(dev, x, y, k, fill=None, want=(True, True, True, True), stream=None, out=None, expect=0):
  """cnf_knn through the C ABI on device tensors x [S, N, D], y [S, M, D] or None: a dict of dist_xx, idx_xx, dist_xy,
  idx_xy (None where not asked for) and sums"""
  from cnf_ot_amd import _capi
  from cnf_ot_amd.flows import _stream_ptr
  S, N, D = x.shape
  M = 0 if y is None else y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_knn_workspace(S, N, M, D, k, ctypes.byref(nbytes)), "cnf_knn_workspace")
  if out is None:
    new = lambda on, dtype: torch.full((S, N, k), 7, dtype=dtype, device=dev) if on else None
    out = {"dist_xx": new(want[0], torch.float32), "idx_xx": new(want[1], torch.int32),
           "dist_xy": new(want[2] and M > 0, torch.float32), "idx_xy": new(want[3] and M > 0, torch.int32),
           "sums": torch.full((S, 2, k, 2), 7.25, dtype=torch.float64, device=dev),
           "ws": torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)}
  if fill is not None:
    out["ws"].fill_(fill)
  assert x.is_contiguous() and x.dtype == torch.float32 and (y is None or (y.is_contiguous() and y.dtype == torch.float32))
  ptr = lambda t: None if t is None else t.data_ptr()
  rc = lib.cnf_knn(S, x.data_ptr(), N, ptr(y), M, D, k, ptr(out["dist_xx"]), ptr(out["idx_xx"]), ptr(out["dist_xy"]),
                   ptr(out["idx_xy"]), out["sums"].data_ptr(), out["ws"].data_ptr(), nbytes.value,
                   _stream_ptr(dev) if stream is None else stream)
  assert rc == expect, rc
  if stream is None:
    torch.cuda.synchronize()
  return out


KEYS = ("dist_xx", "idx_xx", "dist_xy", "idx_xy", "sums")


def _same(a, b, keys=KEYS):
  for key in keys:
    assert (a[key] is None) == (b[key] is None), key
    if a[key] is not None:
      assert torch.equal(a[key], b[key]), key


def _check_exact(got, s, x, y, k, tag):
  """Set s of a call's results against the restatement, bit for bit; the log sums to 1e-10 per mean"""
  N = len(x)
  for b, (block, cloud) in enumerate((("xx", None), ("xy", y))):
    d2, idx = kr.neighbours(x, cloud, k)
    assert np.array_equal(got["idx_" + block][s].cpu().numpy(), idx.astype(np.int32)), (tag, block, "idx")
    assert np.array_equal(got["dist_" + block][s].cpu().numpy().view(np.uint32), kr.dist_f32(d2).view(np.uint32)), (tag, block, "dist")
    want, have = kr.sums_of(d2), got["sums"][s, b].cpu().numpy()
    assert np.array_equal(have[:, 1], want[:, 1]), (tag, block, "zeros")
    err = np.abs(have[:, 0] - want[:, 0]) / np.maximum(N - want[:, 1], 1.0)
    assert err.max() <= 1e-10, (tag, block, err.max())
  return kr.sums_of(kr.neighbours(x, None, k)[0])[:, 1].sum()


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "D%d-N%d-M%d-k%d" % s)
def test_exact_grid_clouds_bit_for_bit(dev, shape):
  D, N, M, k = shape
  index = EXACT_SHAPES.index(shape)
  x, y = kr.exact_grid(D, N, 500 + index), kr.exact_grid(D, M, 600 + index)
  if N > 20:
    x[7], x[N - 1] = x[3], x[3]                            # duplicates: neighbours at distance 0, ordered by index
    y[M - 1] = x[3]
  got = _call(dev, torch.from_numpy(x)[None].to(dev), torch.from_numpy(y)[None].to(dev), k)
  zeros = _check_exact(got, 0, x, y, k, shape)
  assert N <= 20 or zeros > 0


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_knn_splits(1, 64, 64, 3) == 1 and lib.cnf_knn_splits(1, 65, 64, 3) == 2 and lib.cnf_knn_splits(1, 64, 65, 3) == 2
  assert lib.cnf_knn_splits(1, 130, 65, 2) == 3 and lib.cnf_knn_splits(1, 513, 65, 2) == 9
  assert lib.cnf_knn_splits(1, 1025, 1024, 1) == 17 and lib.cnf_knn_splits(1, 700, 0, 2) == 11
  assert lib.cnf_knn_splits(3, 700, 1100, 2) == 18          # 3 sets x 2 blocks x 2 row groups: one tile of 64 columns per split
  src = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "cnf_knn.hip")).read()
  assert "KNN_THREADS = 256;" in src and "KNN_R = 2;" in src and "KNN_TILE = 64;" in src
  assert "KNN_CAP_SMALL = 4;" in src and "KNN_CAP_LARGE = 16;" in src
  assert _capi.KNN_MAX_K == 16 and "#define CNF_KNN_MAX_K 16" in open(
      os.path.join(os.path.dirname(_capi.__file__), "..", "include", "cnf_ot_amd.h")).read()


@pytest.mark.parametrize("case", kr.GAUSSIAN_CASES, ids=lambda c: "D%d-N%d-M%d" % c)
@pytest.mark.parametrize("k", kr.GAUSSIAN_KS)
def test_gaussian_clouds_within_the_float32_bound(dev, case, k):
  D, N, M = case
  x, y = kr.gaussian_case(D, N, M)
  got = _call(dev, torch.from_numpy(x)[None].to(dev), torch.from_numpy(y)[None].to(dev), k)
  bound = kr.distance_bound(D)
  for b, (block, (d2, idx)) in enumerate(zip(("xx", "xy"), kr.gaussian_reference(D, N, M, k))):
    ref = np.sqrt(d2[:, :k])
    dist = got["dist_" + block][0].cpu().double().numpy()
    rel = np.abs(dist - ref) / ref
    keep = kr.index_rule(d2, k, bound)
    same = got["idx_" + block][0].cpu().numpy() == idx[:, :k]
    mean_err = np.abs(got["sums"][0, b, :, 0].cpu().numpy() - kr.sums_of(d2[:, :k])[:, 0]) / N
    print(f"\n[knn D={D} N={N} M={M} k={k} {block}] dist rel err {rel.max():.2e} (bound {bound:.2e}), log mean err "
          f"{mean_err.max():.2e}, indices compared {keep.mean():.4f}, equal {same.mean():.4f}")
    assert rel.max() <= bound
    assert mean_err.max() <= bound + 1e-12
    assert keep.mean() >= 0.99 and same[keep].all()
    assert bool((got["sums"][0, b, :, 1] == 0).all())


def test_rank_j_does_not_depend_on_k(dev):
  x, y = kr.gaussian_case(3, 257, 130)
  g = kr.exact_grid(2, 300, 77)
  for xs, ys in ((x, y), (g, g[:140].copy())):
    xd, yd = torch.from_numpy(xs)[None].to(dev), torch.from_numpy(ys)[None].to(dev)
    full = _call(dev, xd, yd, 16)
    for j in (1, 4, 5):
      part = _call(dev, xd, yd, j)
      for key in KEYS:
        assert torch.equal(full[key][:, :, :j] if key != "sums" else full[key][:, :, :j, :], part[key]), (j, key)


def test_the_self_block_is_the_cross_block_against_a_copy_shifted_by_one_rank(dev):
  for x in (kr.gaussian(3, 700, 8), kr.gaussian(10, 130, 9)):
    xd = torch.from_numpy(x)[None].to(dev)
    got = _call(dev, xd, xd.clone(), 6)
    N = x.shape[0]
    assert torch.equal(got["idx_xy"][0, :, 0].cpu(), torch.arange(N, dtype=torch.int32)) and bool((got["dist_xy"][0, :, 0] == 0).all())
    assert torch.equal(got["dist_xy"][:, :, 1:], got["dist_xx"][:, :, :5]) and torch.equal(got["idx_xy"][:, :, 1:], got["idx_xx"][:, :, :5])
    assert torch.equal(got["sums"][:, 1, 1:, :], got["sums"][:, 0, :5, :])
    assert got["sums"][0, 1, 0].tolist() == [0.0, float(N)]


def test_three_sets_with_their_own_data(dev):
  D, N, M, k, S = 2, 257, 130, 5, 3
  x, y = kr.exact_grid(D, N, 40, S=S), kr.exact_grid(D, M, 41, S=S)
  got = _call(dev, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), k)
  for s in range(S):
    _check_exact(got, s, x[s], y[s], k, f"set {s}")
  assert len({tuple(got["sums"][s].flatten().tolist()) for s in range(S)}) == S      # three different answers: no set read twice


def test_reproducibility(dev):
  D, N, M, k, S = 3, 700, 1100, 7, 2
  x = torch.from_numpy(kr.gaussian(D, N, 50, S=S)).to(dev)
  y = torch.from_numpy(kr.gaussian(D, M, 51, mean=0.5, scale=1.25, S=S)).to(dev)
  base = _call(dev, x, y, k)
  assert all(bool(torch.isfinite(base[key].double()).all()) for key in KEYS)
  _same(base, _call(dev, x, y, k))                                    # two calls
  _same(base, _call(dev, x, y, k, fill=0xFF))                         # (0xFF bytes: NaN / -1 wherever a word is read before it is written)
  # inputs at 4-byte-but-not-16-byte offsets
  xo, yo = torch.empty(x.numel() + 1, device=dev), torch.empty(y.numel() + 3, device=dev)
  xs, ys = xo[1:].view_as(x).copy_(x), yo[3:].view_as(y).copy_(y)
  assert xs.data_ptr() % 16 == 4 and ys.data_ptr() % 16 == 12
  _same(base, _call(dev, xs, ys, k))
  # one call replayed from a captured graph: a single stream, one linear chain of launches, nothing allocated
  replay = _call(dev, x, y.flip(0).contiguous(), k)
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    _call(dev, x, y, k, stream=side.cuda_stream, out=replay)
  for key in KEYS:
    replay[key].fill_(7)
  graph.replay()
  torch.cuda.synchronize()
  _same(base, replay)


def test_optional_outputs_and_the_self_block_alone(dev):
  D, N, M, k = 2, 513, 65, 5
  x = torch.from_numpy(kr.gaussian(D, N, 60))[None].to(dev)
  y = torch.from_numpy(kr.gaussian(D, M, 61))[None].to(dev)
  base = _call(dev, x, y, k)
  for want in ((False, False, False, False), (True, False, False, True), (False, True, True, False)):
    got = _call(dev, x, y, k, want=want)
    _same(base, got, [key for key, on in zip(KEYS, want + (True,)) if on])
    assert all(got[key] is None for key, on in zip(KEYS, want) if not on)
  alone = _call(dev, x, None, k)
  _same(base, alone, ("dist_xx", "idx_xx"))
  assert torch.equal(alone["sums"][:, 0], base["sums"][:, 0]) and bool((alone["sums"][:, 1] == 0).all())
  # one byte too few: refused, nothing written
  from cnf_ot_amd import _capi
  nbytes = ctypes.c_int64(0)
  _capi.lib().cnf_knn_workspace(1, N, M, D, k, ctypes.byref(nbytes))
  sums = torch.full((1, 2, k, 2), 7.25, dtype=torch.float64, device=dev)
  ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
  assert _capi.lib().cnf_knn(1, x.data_ptr(), N, y.data_ptr(), M, D, k, None, None, None, None, sums.data_ptr(), ws.data_ptr(),
                             nbytes.value - 1, None) == _capi.CNF_ERR_INVALID
  torch.cuda.synchronize()
  assert bool((sums == 7.25).all()) and not bool(ws.any())


# ---- the Python surface at N = 5, M = 7, D = 3: the table of test_gpu_two_sample_surface.py, stated for knn ----------

SN, SM, SD = 5, 7, 3
PER_POINT = ("dist_xx", "dist_xy", "idx_xx", "idx_xy")


def _data(S):
  rng = np.random.default_rng(40 + S)
  return rng.standard_normal((S, SN, SD)), 0.5 + 1.25 * rng.standard_normal((S, SM, SD))


def _knn(x, y):
  from cnf_ot_amd import utils
  res = utils.knn(x, y, k=3, want_indices=True)
  torch.cuda.synchronize()
  return res


def _same_bits(a, b):
  assert set(a) == set(b)
  for key in a:
    assert a[key].dtype == b[key].dtype and a[key].device == b[key].device and torch.equal(a[key], b[key]), key


def _on(dev, t):
  return torch.from_numpy(t).to(device=dev, dtype=torch.float32)


def test_surface_a_2d_x_against_the_same_set_as_3d(dev):
  x, y = _data(1)
  two, three = _knn(x[0], y[0]), _knn(x, y)
  for key in PER_POINT:
    assert two[key].shape == (SN, 3) and three[key].shape == (1, SN, 3)
    two[key] = two[key][None]
  _same_bits(two, three)
  assert three["sums"].shape == (1, 2, 3, 2) and three["idx_xx"].dtype == torch.int32
  from cnf_ot_amd import utils
  plain = utils.knn(x, None, k=3)
  assert set(plain) == {"dist_xx", "dist_xy", "sums"} and plain["dist_xy"] is None and torch.equal(plain["dist_xx"], three["dist_xx"])


@pytest.mark.parametrize("S", [1, 2])
def test_surface_host_float64_against_float32_on_the_device(dev, S):
  x, y = _data(S)
  host, there = _knn(x, y), _knn(_on(dev, x), _on(dev, y))
  assert all(v.is_cuda for v in host.values())
  _same_bits(host, there)
  yd = _on(dev, y)
  _same_bits(_knn(torch.from_numpy(x), yd), there)          # x on the host and y on the device


@pytest.mark.parametrize("S", [1, 2])
def test_surface_views_against_their_contiguous_copies(dev, S):
  x, y = _data(S)
  xv = _on(dev, np.ascontiguousarray(x.transpose(0, 2, 1))).transpose(1, 2)      # [S, N, D], a view of [S, D, N]
  yv = _on(dev, y[:1]).expand(S, -1, -1)                                           # one set, S times
  assert not xv.is_contiguous() and yv.is_contiguous() == (S == 1)
  _same_bits(_knn(xv, yv), _knn(xv.contiguous(), yv.contiguous()))
  res = _knn(xv.clone().requires_grad_(True), yv)
  assert all(v.grad_fn is None and not v.requires_grad for v in res.values())


# ---- estimators and evaluation ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(2, 700, 1100), (10, 300, 257)], ids=lambda c: "D%d-N%d-M%d" % c)
def test_knn_divergence_against_the_restatement(dev, case):
  from cnf_ot_amd import utils
  D, N, M = case
  k = 4
  x, y = kr.gaussian_case(D, N, M)
  got = utils.knn_divergence(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), k)
  (dxx, _), (dxy, _) = kr.gaussian_reference(D, N, M, k)
  want = kr.estimates(np.stack([kr.sums_of(dxx[:, :k]), kr.sums_of(dxy[:, :k])]), N, M, D)
  bound = D * (kr.distance_bound(D) + 1e-12)
  for key in ("entropy", "cross_entropy", "kl"):
    err = np.abs(got["by_rank"][key][0].cpu().numpy() - want[key]).max()
    print(f"\n[knn_divergence D={D} N={N} M={M}] {key} {want[key][-1]:.4f} err {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert got[key].shape == (1,) and got[key][0].item() == got["by_rank"][key][0, -1].item()
  assert got["k"] == k and not bool(got["zeros"].any())
  ent = utils.knn_entropy(torch.from_numpy(x).to(dev), k)
  assert torch.equal(ent["entropy"], got["entropy"]) and ent["by_rank"]["kl"] is None


FP_CASES = [("ou", 2), ("lorenz", 3)]


@pytest.mark.parametrize("sub,dim", FP_CASES)
def test_evaluate_fp_knn_is_its_composition(dev, sub, dim):
  from cnf_ot_amd import FlowConfig, Params, applications, solvers, utils
  from cnf_ot_amd.distributed import Shard
  cfg = solvers.load_config(overrides={"general": {"type": "fp", "dim": dim}, "fp": {"velocity_field_type": sub}})
  model = solvers.build_model(cfg)
  params = Params.random(FlowConfig(dim=dim), 0.2, seed=4, device=dev)
  n_particles, h, seed, k = 4096, 1e-2, 5, 4
  res = solvers.evaluate_fp_knn(cfg, model, params, n_particles=n_particles, h=h, seed=seed, k=k)
  assert set(res) == set(solvers.FP_KNN_KEYS) and res["n"] == n_particles // 2 and res["k"] == k
  ts = res["times"]
  f = cfg["fp"]
  h0, h1 = (applications.fp_reference_particles(dim, f["T"], f["a"], f["sigma"], sub, np.asarray(ts), n_particles, h, seed,
                                                positions=True, shard=Shard(r, 2), all_reduce=False)["pos"].float() for r in (0, 1))
  want = {key: [] for key in solvers.FP_KNN_KEYS[1:7]}
  for i, t in enumerate(ts):
    y, lp = model.apply.sample_and_log_prob(params, cond=float(t), seed=seed, sample_shape=(n_particles // 2,))
    fwd, floor, rev = utils.knn_divergence(y, h0[i], k), utils.knn_divergence(h1[i], h0[i], k), utils.knn_divergence(h0[i], y, k)
    want["kl"].append(fwd["kl"].item())
    want["kl_floor"].append(floor["kl"].item())
    want["kl_reverse"].append(rev["kl"].item())
    want["entropy_knn"].append(fwd["entropy"].item())
    want["entropy_model"].append(-lp.double().mean().item())
    want["kl_ensemble_flow"].append(-rev["entropy"].item() - model.apply.log_prob(params, h0[i], cond=float(t)).double().mean().item())
  for key, v in want.items():
    assert np.array_equal(np.array(res[key]), np.array(v), equal_nan=True), key
    assert np.isfinite(res[key][0]), key
  solvers.print_fp_knn(res)


def test_an_identity_flow_stands_out_of_the_floor(dev):
  """T = 3: the ensemble starts from N(0, (T + 1) / 2 I) = N(0, 2 I); the identity flow samples N(0, I), and in dim 2
  KL(N(0, I) || N(0, 2 I)) = log 2 - 1 / 2 = 0.193 nats.  The bars: at 2 048 points per set the estimate's sampling
  standard error is about 0.016 sqrt 2 = 0.023 and its bias within 0.035 (the figures of tests/test_knn_cpu.py at 4 096
  points), so 3 standard errors and the bias are 0.1; the difference kl - kl_floor has the standard error 0.033 and
  stays above 0.193 - 0.1 - 0.035 > 0.05.  The entropy of N(0, I) in dim 2 is log(2 pi e) = 2.838."""
  from cnf_ot_amd import FlowConfig, Params, solvers
  cfg = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou", "T": 3.0}})
  model = solvers.build_model(cfg)
  res = solvers.evaluate_fp_knn(cfg, model, Params.zeros(FlowConfig(dim=2), dev), times=[0.0, 0.1], n_particles=4096, h=1e-2, seed=5)
  solvers.print_fp_knn(res)
  kl, floor = res["kl"][0], res["kl_floor"][0]
  assert abs(kl - 0.193) <= 0.1 and abs(floor) <= 0.1 and kl - floor > 0.05
  assert abs(res["entropy_knn"][0] - 2.838) <= 0.1 and abs(res["entropy_model"][0] - 2.838) <= 0.1
