"""What utils.mmd2, utils.sinkhorn and utils.sliced_wasserstein do with their inputs before the kernel runs -- the part
they share (cnf_ot_amd/two_sample.py: the sets as [S, N, D], the device, float32, contiguity, the result of a 2-D x) --
one table over the three statistics at the smallest shapes that pass through it: S 1 and 2, N 5, M 7, D 3.  Every
comparison is of bits: the staging decides what the kernel reads, not what it computes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, M, D = 5, 7, 3
PER_POINT = ("grad", "map")      # [S, N, D] entries: [N, D] for a 2-D x


def _directions():
  from cnf_ot_amd import utils
  return utils.sliced_directions(D, 4, seed=3)


STATS = {
    "mmd-gaussian": lambda u, x, y: u.mmd2(x, y, [0.7, 1.5], "gaussian", want_grad=True),
    "mmd-energy": lambda u, x, y: u.mmd2(x, y, None, "energy", want_grad=True),
    "sinkhorn": lambda u, x, y: u.sinkhorn(x, y, schedule=[1.0, 0.5], want_grad=True, want_map=True, want_potentials=True),
    "sliced": lambda u, x, y: u.sliced_wasserstein(x, y, _directions(), want_grad=True),
}
stat = pytest.mark.parametrize("name", sorted(STATS))
sets = pytest.mark.parametrize("S", [1, 2])


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _data(S):
  """(x [S, N, D], y [S, M, D]) float64 on the host, a fixed function of S"""
  rng = np.random.default_rng(40 + S)
  return rng.standard_normal((S, N, D)), 0.5 + 1.25 * rng.standard_normal((S, M, D))


def _call(name, x, y):
  from cnf_ot_amd import utils
  res = STATS[name](utils, x, y)
  torch.cuda.synchronize()
  return res


def _same_bits(a, b):
  assert set(a) == set(b)
  for k in a:
    if torch.is_tensor(a[k]):
      assert a[k].dtype == b[k].dtype and a[k].device == b[k].device and torch.equal(a[k], b[k]), k
    else:
      assert a[k] == b[k], k      # (None, or a list of floats)


def _on(dev, t):
  return torch.from_numpy(t).to(device=dev, dtype=torch.float32)


@stat
def test_a_2d_x_against_the_same_set_as_3d(dev, name):
  x, y = _data(1)
  two, three = _call(name, x[0], y[0]), _call(name, x, y)
  for k in PER_POINT:
    if k in three:
      assert two[k].shape == (N, D) and three[k].shape == (1, N, D)
      two[k] = two[k][None]
  _same_bits(two, three)


@stat
@sets
def test_host_float64_against_float32_on_the_device(dev, name, S):
  x, y = _data(S)
  host, there = _call(name, x, y), _call(name, _on(dev, x), _on(dev, y))
  assert all(v.is_cuda for v in host.values() if torch.is_tensor(v))
  _same_bits(host, there)


@stat
def test_x_on_the_host_and_y_on_the_device(dev, name):
  x, y = _data(2)
  yd = _on(dev, y)
  mixed = _call(name, torch.from_numpy(x), yd)
  assert all(v.device == yd.device for v in mixed.values() if torch.is_tensor(v))
  _same_bits(mixed, _call(name, _on(dev, x), yd))


@stat
@sets
def test_views_against_their_contiguous_copies(dev, name, S):
  x, y = _data(S)
  xv = _on(dev, np.ascontiguousarray(x.transpose(0, 2, 1))).transpose(1, 2)      # [S, N, D], a view of [S, D, N]
  yv = _on(dev, y[:1]).expand(S, -1, -1)                                           # one set, S times
  assert not xv.is_contiguous() and yv.is_contiguous() == (S == 1)
  _same_bits(_call(name, xv, yv), _call(name, xv.contiguous(), yv.contiguous()))
  if S == 1:      # ... and the 2-D view of a [D, N] tensor
    _same_bits(_call(name, xv[0], yv[0]), _call(name, xv[0].contiguous(), yv[0]))


@stat
@sets
def test_an_x_that_requires_grad(dev, name, S):
  x, y = _data(S)
  xd, yd = _on(dev, x), _on(dev, y)
  res = _call(name, xd.clone().requires_grad_(True), yd)
  assert all(v.grad_fn is None and not v.requires_grad for v in res.values() if torch.is_tensor(v))
  _same_bits(res, _call(name, xd, yd))
