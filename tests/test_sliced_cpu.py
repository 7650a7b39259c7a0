"""CPU tests of the sliced Wasserstein distance: the float64 restatement (tests/sliced_ref.py) the GPU tests hold
cnf_sliced_w2 to is pinned by facts that do not come from it, then utils.sliced_directions, the host-side argument checks
of cnf_sliced_w2 through the C ABI (no device is touched) and the Python entry points' refusals, which come before any
device work.

Measured (every test prints its figures: run with -s):
  unequal sizes against lcm replication      largest relative difference 2.2e-16 over (3, 5) (4, 6) (1, 7) (7, 1) (64, 48)
  translation, D = 3, N = 257, P = 5         values within 0.0 of (theta.c)^2 / 2, N grad within 2.2e-16 (bar 1e-12)
  gradient against central differences       5.6e-10 relative on N grad of size 1.96 (bar 1e-6), D = 2, N = 40, M = 30
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliced_ref as sl


def _keys_1d(n, seed):
  return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def test_equal_sizes_are_the_sorted_pairing():
  kx, ky = _keys_1d(257, 1), _keys_1d(257, 2) * 1.5 + 0.25
  w, a, px, py = sl.one(kx, ky)
  sx, sy = np.sort(kx.astype(np.float64)), np.sort(ky.astype(np.float64))
  assert abs(w - 0.5 * np.mean((sx - sy) ** 2)) <= 1e-15 * w
  assert np.array_equal(kx[px], np.sort(kx)) and np.array_equal(ky[py], np.sort(ky))
  # a at the rank a sample took: (k_(i) - l_(i)) / N
  assert np.abs(a[px] - (sx - sy) / 257).max() <= 1e-17


@pytest.mark.parametrize("N,M", [(3, 5), (4, 6), (1, 7), (7, 1), (64, 48)])
def test_unequal_sizes_are_the_pairing_of_the_replicated_keys(N, M):
  kx, ky = _keys_1d(N, 10 + N), _keys_1d(M, 20 + M) + 0.5
  w, a, px, _ = sl.one(kx, ky)
  L = math.lcm(N, M)
  rx, ry = np.repeat(np.sort(kx.astype(np.float64)), L // N), np.repeat(np.sort(ky.astype(np.float64)), L // M)
  want = 0.5 * np.mean((rx - ry) ** 2)
  print(f"\n[sliced lcm N={N} M={M}] w {w:.12f} against {want:.12f}: {abs(w - want) / want:.1e}")
  assert abs(w - want) <= 1e-14 * want
  a_want = ((rx - ry) / L).reshape(N, L // N).sum(1)
  assert np.abs(a[px] - a_want).max() <= 1e-15
  # the header's o_ij, pair by pair, says the same
  sx, sy = np.sort(kx.astype(np.float64)), np.sort(ky.astype(np.float64))
  direct = 0.5 * sum(sl.overlap(i, j, N, M) * (sx[i] - sy[j]) ** 2 for i in range(N) for j in range(M))
  assert abs(direct - want) <= 1e-14 * want
  # ... and rank i meets the ranks floor(i M / N) .. floor(((i + 1) M - 1) / N) and no other
  for i in range(N):
    met = [j for j in range(M) if sl.overlap(i, j, N, M) > 0]
    assert met == list(range(i * M // N, ((i + 1) * M - 1) // N + 1))
    assert abs(sum(sl.overlap(i, j, N, M) for j in met) - 1.0 / N) <= 2.0 ** -52 * len(met) / N      # (len(met) rounded quotients)


def test_translation():
  """y = x + c on the exact grid: every projected pair differs by theta.c, so w = (theta.c)^2 / 2 and
  N grad = -(1 / P) sum_p (theta_p.c) theta_p"""
  D, N, P = 3, 257, 5
  x, _ = sl.clouds_exact(D, N, 1, seed=3)
  c = np.array([1.5, -0.75, 0.25], dtype=np.float32)
  theta = sl.directions_exact(D, P, seed=3)
  r = sl.run(x, x + c, theta)
  tc = theta.astype(np.float64) @ c.astype(np.float64)
  e_w = np.abs(r["w"] - 0.5 * tc * tc).max()
  want = (tc[:, None] * theta.astype(np.float64)).sum(0) / P
  e_g = np.abs(r["grad"] * N + want[None, :]).max()          # (k - l = -theta.c: descent moves x towards y)
  print(f"\n[sliced translation] values within {e_w:.1e}, N grad within {e_g:.1e}")
  assert e_w <= 1e-12 and e_g <= 1e-12
  assert abs(r["sw"] - np.mean(0.5 * tc * tc)) <= 1e-12 and abs(r["max_sliced"] - (0.5 * tc * tc).max()) <= 1e-12


def test_a_cloud_against_itself_symmetry_and_repeated_directions():
  D, N, M, P = 3, 130, 77, 4
  x, y = sl.clouds(D, N, M, seed=5)
  theta = sl.directions_exact(D, P, seed=5)
  same = sl.run(x, x.copy(), theta)
  assert (same["w"] == 0.0).all() and same["sw"] == 0.0 and (same["grad"] == 0.0).all()
  fwd, back = sl.run(x, y, theta), sl.run(y, x, theta)
  assert np.abs(fwd["w"] - back["w"]).max() <= 1e-15 * fwd["w"].max()
  twice = sl.run(x, y, np.stack([theta[1], theta[1]]))
  assert twice["w"][0] == twice["w"][1] == fwd["w"][1] and abs(twice["sw"] - fwd["w"][1]) <= 1e-16
  assert np.abs(twice["grad"] - fwd["a"][1][:, None] * theta[1].astype(np.float64)[None, :]).max() <= 1e-16


def test_gradient_against_central_differences():
  """On the exact grid the float32 keys are the float64 ones; with distinct keys a step of 1e-6 (grid spacing of a key:
  2^-16) changes no permutation, and the value is quadratic in the step: the central difference is exact up to rounding"""
  D, N, M, P = 2, 40, 30, 4
  x, y = sl.clouds_exact(D, N, M, seed=7)
  theta = sl.directions_exact(D, P, seed=7)
  r = sl.run(x, y, theta)
  for p in range(P):
    assert len(np.unique(r["kx"][p])) == N and len(np.unique(r["ky"][p])) == M      # tie-free
  g = r["grad"] * N
  h, worst = 1e-6, 0.0
  x64 = x.astype(np.float64)
  for i in (0, 7, 19, N - 1):
    for d in range(D):
      xp, xm = x64.copy(), x64.copy()
      xp[i, d] += h
      xm[i, d] -= h
      fd = (sl.value64(xp, y, theta) - sl.value64(xm, y, theta)) / (2.0 * h) * N
      worst = max(worst, abs(fd - g[i, d]))
  scale = np.abs(g).max()
  print(f"\n[sliced gradient] central differences: {worst / scale:.1e} relative on N grad of size {scale:.2f}")
  assert worst <= 1e-6 * scale
  assert abs(sl.value64(x64, y, theta) - r["sw"]) <= 1e-14 * r["sw"]


def test_the_axes_give_every_marginal():
  D, N = 3, 200
  x, y = sl.clouds(D, N, N, seed=9)
  r = sl.run(x, y, np.eye(D, dtype=np.float32))
  for d in range(D):
    want = 0.5 * np.mean((np.sort(x[:, d].astype(np.float64)) - np.sort(y[:, d].astype(np.float64))) ** 2)
    assert abs(r["w"][d] - want) <= 1e-15 * want


def test_ties_go_by_index_and_non_finite_keys_are_nan():
  k = np.array([1.0, -0.0, 1.0, 0.0, -2.0, 1.0], dtype=np.float32)
  assert sl.order(k).tolist() == [4, 1, 3, 0, 2, 5]
  x = np.array([[1.0, 2.0], [np.inf, 0.0], [0.5, np.nan]], dtype=np.float32)
  kk = sl.keys(x, np.array([[1.0, 0.0], [0.5, 0.5]], dtype=np.float32))
  assert np.isnan(kk[:, 1:]).all() and kk[:, 0].tolist() == [1.0, 1.5]
  r = sl.run(x, x[:1], np.array([[1.0, 0.0]], dtype=np.float32))
  assert np.isnan(r["sums"]).all() and np.isnan(r["grad"]).all()


@pytest.mark.parametrize("D", sorted(sl.ORDINARY))
def test_the_ordinary_cases_leave_few_rows_to_rounding(D):
  """The GPU test compares the gradient only on rows whose ranks agree between the restatement (fused keys) and a
  float32 composition (a matrix product's keys): for the seeds chosen that must leave out less than 1 % of the rows"""
  from cnf_ot_amd import utils
  N, M, P, seed = sl.ORDINARY[D]
  x, y = sl.clouds(D, N, M, seed)
  theta = utils.sliced_directions(D, P, seed).numpy()
  r = sl.run(x, y, theta)
  kx32 = (x @ theta.T).T.astype(np.float32)
  other = np.stack([np.argsort(k, kind="stable") for k in kx32])
  share = 1.0 - sl.rows_that_agree(r["perm_x"], other).mean()
  print(f"\n[sliced ordinary D={D}] rows of x whose rank differs under a float32 product's keys: {100 * share:.3f} %")
  assert share < 0.01


def test_directions():
  from cnf_ot_amd import utils
  th = utils.sliced_directions(5, 64, seed=3)
  assert tuple(th.shape) == (64, 5) and str(th.dtype) == "torch.float32" and not th.is_cuda
  assert np.abs(np.linalg.norm(th.numpy().astype(np.float64), axis=1) - 1.0).max() <= 1e-6
  assert np.array_equal(th.numpy(), utils.sliced_directions(5, 64, seed=3).numpy())
  assert not np.array_equal(th.numpy(), utils.sliced_directions(5, 64, seed=4).numpy())
  assert utils.sliced_directions(1, 1).tolist() == [[1.0]]
  assert np.array_equal(utils.sliced_directions(3, 3, kind="axes").numpy(), np.eye(3, dtype=np.float32))
  for bad in ((0, 4, {}), (15, 4, {}), (2, 0, {}), (2, 1025, {}), (1, 2, {}), (3, 2, {"kind": "axes"}), (3, 3, {"kind": "sobol"})):
    with pytest.raises(ValueError):
      utils.sliced_directions(bad[0], bad[1], **bad[2])


def test_the_c_abi_refuses_before_the_device():
  """Every rejection of cnf_sliced_w2 and cnf_sliced_workspace comes back CNF_ERR_INVALID on a machine without a GPU;
  the buffers are host memory that no rejected call may read or write: they keep their fill."""
  from cnf_ot_amd import _capi
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  T = lib.cnf_sliced_tile()
  assert T >= 2048 and T & (T - 1) == 0
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_sliced_workspace(3, 300, 257, 10, 4, 1, ctypes.byref(nbytes)) == _capi.CNF_OK
  R = 3 * 4
  assert nbytes.value == 2 * R * 557 * 8 + R * 2 * 8 + R * 300 * 8 + 3 * 300 * 10 * 8
  small = ctypes.c_int64(-1)
  for bad in ((0, 300, 257, 10, 4), (65, 300, 257, 10, 4), (3, 0, 257, 10, 4), (3, 300, 0, 10, 4), (3, 300, 257, 0, 4),
              (3, 300, 257, 15, 4), (3, (1 << 20) + 1, 257, 2, 4), (3, 300, (1 << 20) + 1, 2, 4), (3, 300, 257, 10, 0),
              (3, 300, 257, 10, 1025)):
    assert lib.cnf_sliced_workspace(*bad, 1, ctypes.byref(small)) == INV, bad
  assert small.value == -1 and lib.cnf_sliced_workspace(3, 300, 257, 10, 4, 1, None) == INV

  # monotone in G and in want_grad
  def size(G, wg, shape=(3, 300, 257, 10)):
    b = ctypes.c_int64(0)
    assert lib.cnf_sliced_workspace(*shape, G, wg, ctypes.byref(b)) == _capi.CNF_OK
    return b.value
  for wg in (0, 1):
    sizes = [size(G, wg) for G in (1, 2, 3, 7, 64, 1024)]
    assert all(a < b for a, b in zip(sizes[:-1], sizes[1:]))
    assert size(2, wg) - size(1, wg) == size(3, wg) - size(2, wg)        # linear: what utils.sliced_group relies on
  assert all(size(G, 0) < size(G, 1) for G in (1, 5, 1024))
  assert size(1, 0, (64, 1 << 20, 1 << 20, 14)) > 0

  f32, f64 = np.full(3 * 300 * 10, 7.25, np.float32), np.full(3 * 10, 7.25, np.float64)
  ws = np.full(64, 7.25, np.float64)
  p, d, w = f32.ctypes.data, f64.ctypes.data, ws.ctypes.data
  good = dict(S=3, x=p, N=300, y=p, M=257, D=10, theta=p, P=8, G=4, sums=d, grad=p, ws=w, wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_sliced_w2(a["S"], a["x"], a["N"], a["y"], a["M"], a["D"], a["theta"], a["P"], a["G"], a["sums"], a["grad"],
                             a["ws"], a["wsb"], None)

  bad = [{"x": None}, {"y": None}, {"theta": None}, {"sums": None}, {"ws": None}, {"S": 0}, {"S": 65}, {"D": 0}, {"D": 15},
         {"N": 0}, {"M": 0}, {"N": -1}, {"N": (1 << 20) + 1}, {"M": (1 << 20) + 1}, {"P": 0}, {"P": 1025}, {"G": 0}, {"G": -1},
         {"G": 9}, {"P": 3}, {"wsb": nbytes.value - 1}, {"wsb": 0}, {"grad": None, "wsb": size(4, 0) - 1}]
  wrong = {str(k): call(**k) for k in bad}
  wrong = {k: v for k, v in wrong.items() if v != INV}
  assert not wrong, wrong
  assert (f32 == 7.25).all() and (f64 == 7.25).all() and (ws == 7.25).all()


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import applications as app, solvers, utils
  from cnf_ot_amd.distributed import Shard
  utils.sliced_check_shapes((3, 5, 2), (3, 7, 2), (64, 2))
  for bad in (((3, 5, 2), (2, 7, 2), None), ((3, 5, 2), (3, 7, 3), None), ((0, 5, 2), (0, 7, 2), None),
              ((65, 5, 2), (65, 7, 2), None), ((1, 0, 2), (1, 7, 2), None), ((1, 5, 2), (1, 0, 2), None),
              ((1, (1 << 20) + 1, 2), (1, 7, 2), None), ((1, 5, 15), (1, 7, 15), None), ((1, 5, 2), (1, 7, 2), (4, 3)),
              ((1, 5, 2), (1, 7, 2), (0, 2)), ((1, 5, 2), (1, 7, 2), (1025, 2)), ((1, 5, 2), (1, 7, 2), (2,))):
    with pytest.raises(ValueError):
      utils.sliced_check_shapes(*bad)
  x, y = np.zeros((5, 3), dtype=np.float32), np.ones((7, 3), dtype=np.float32)
  for bad in ({"y": np.ones((7, 2), dtype=np.float32)}, {"x": np.zeros(5)}, {"directions": np.ones((4, 2))},
              {"x": np.zeros((2, 5, 3)), "y": np.ones((3, 7, 3))}, {"n_proj": 0}, {"n_proj": 1025},
              {"x": np.zeros((5, 15)), "y": np.ones((7, 15))}):
    with pytest.raises(ValueError):
      utils.sliced_wasserstein(**dict(dict(x=x, y=y), **bad))
  tgt = np.ones((130, 2), dtype=np.float32)
  with pytest.raises(ValueError):
    app.sliced_loss_fn(None, 2, None, tgt, [0.5], 0, 96, shard=Shard(0, 2))
  for kw in ({"target": np.ones((130, 3), dtype=np.float32)}, {"batch_size": 0}, {"target": np.ones((2, 130, 2))},
             {"directions": np.ones((4, 3))}, {"n_proj": 2000}, {"target": np.ones(130)}):
    a = dict(dict(target=tgt, batch_size=96, directions=None, n_proj=64), **kw)
    with pytest.raises(ValueError):
      app.sliced_loss_fn(None, 2, None, a["target"], [0.5], 0, a["batch_size"], directions=a["directions"], n_proj=a["n_proj"],
                         shard=Shard(0, 1))
  for over in ({"general": {"type": "rwpo"}}, {"general": {"type": "ot", "dim": 2}}):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_sliced(solvers.load_config(overrides=over), None, None)
  assert solvers._parse(["--sliced"]).sliced and not solvers._parse([]).sliced
  with pytest.raises(ValueError):      # (the checked-in default is rwpo: refused before any training step)
    solvers.main(solvers.load_config(), sliced=True)
