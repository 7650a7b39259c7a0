"""Checks of tests/stein_ref.py itself -- the float64 restatement cnf_stein is held to -- against torch float64 autograd
of the DEFINITION (the Stein operator applied to the base kernel, not the closed form), and of what the Python layer
refuses before any device work.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stein_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = {"imq/1": sr.spec("imq", [1.0]), "imq/2": sr.spec("imq", [0.5, 2.0], [1.0, 0.25], beta=-0.75),
         "imq/4": sr.spec("imq", [0.5, 1.0, 2.0, 4.0], [1.0, 0.5, 0.25, 2.0], beta=-0.25),
         "gaussian/1": sr.spec("gaussian", [1.5]), "gaussian/3": sr.spec("gaussian", [0.5, 1.0, 3.0], [1.0, 0.5, 0.25]),
         "gaussian/4": sr.spec("gaussian", [0.5, 1.0, 2.0, 4.0], [0.25, 1.0, 0.5, 2.0])}


def _phi(q, sp):
  """phi(q) in torch float64, written from the kinds' definitions"""
  out = 0.0
  for w, bw in zip(sp["w"], sp["bw"]):
    out = out + (w * (bw * bw + q) ** sp["beta"] if sp["kind"] == "imq" else w * torch.exp(-q / (2.0 * bw * bw)))
  return out


def _stein_kernel(xa, xb, sa, sb, sp):
  """k_p(x, y) from its definition: s_x . s_y k + s_x . grad_y k + s_y . grad_x k + tr grad_x grad_y k, by autograd"""
  xa, xb = xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)
  k = _phi(((xa - xb) ** 2).sum(), sp)
  gx, gy = torch.autograd.grad(k, (xa, xb), create_graph=True)
  tr = sum(torch.autograd.grad(gx[a], xb, create_graph=True)[0][a] for a in range(len(xa)))
  return k * (sa @ sb) + sa @ gy + sb @ gx + tr


def _ksd_u(x, s, sp):
  N = len(x)
  return sum(_stein_kernel(x[i], x[j], s[i], s[j], sp) for i in range(N) for j in range(N) if i != j) / (N * (N - 1.0))


def _inputs(D, N, seed):
  x = sr.cloud(D, N, seed, 1.25).astype(np.float64)
  s = -x + 0.3 * sr.cloud(D, N, seed + 1).astype(np.float64)
  return x, s


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("D", [1, 3])
def test_the_restatement_is_the_definition(name, D):
  sp, N = SPECS[name], 5
  x, s = _inputs(D, N, 10 + D)
  ref = sr.stats(x, s, sp)
  xt, st = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(s).requires_grad_(True)
  # values: every pair, and the rows and sums they make
  kp = [[float(_stein_kernel(xt[i].detach(), xt[j].detach(), st[i].detach(), st[j].detach(), sp).detach()) for j in range(N)]
        for i in range(N)]
  kp = np.array(kp)
  off = kp - np.diag(np.diag(kp))
  tol = 1e-12 * max(1.0, np.abs(kp).max())
  assert abs(ref["sums"][0] - off.sum()) <= N * N * tol
  assert np.abs(ref["rows"] - off.sum(1) / (N - 1.0)).max() <= N * tol
  # the diagonal formula: the definition at x = y
  assert abs(ref["sums"][1] - np.trace(kp)) <= N * tol
  u, v = sr.ksd2(x, s, sp)
  assert abs(u - off.sum() / (N * (N - 1.0))) <= tol and abs(v - kp.sum() / (N * N)) <= tol
  # gradients: autograd of the definition's U statistic, s an independent input
  gx, gs = torch.autograd.grad(_ksd_u(xt, st, sp), (xt, st))
  gtol = 1e-11 * max(1.0, float(gx.abs().max()), float(gs.abs().max()))
  assert np.abs(ref["grad_x"] - gx.numpy()).max() <= gtol
  assert np.abs(ref["grad_s"] - gs.numpy()).max() <= gtol


@pytest.mark.parametrize("name", ["imq/2", "gaussian/3"])
def test_direction_is_its_definition(name):
  sp, N, D = SPECS[name], 6, 2
  x, s = _inputs(D, N, 20)
  ref = sr.stats(x, s, sp)
  xt, st = torch.from_numpy(x), torch.from_numpy(s)
  want = np.zeros((N, D))
  for i in range(N):
    for j in range(N):
      xj = xt[j].clone().requires_grad_(True)
      k = _phi(((xj - xt[i]) ** 2).sum(), sp)
      want[i] += (k.detach() * st[j] + torch.autograd.grad(k, xj)[0]).numpy() / N
  assert np.abs(ref["direction"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_the_float32_composition_is_close_and_not_equal():
  sp = SPECS["imq/4"]
  x, s = _inputs(3, 40, 30)
  a, b = sr.stats(x, s, sp), sr.stats(x, s, sp, dtype=np.float32)
  e = np.abs(a["rows"] - b["rows"]).max()
  assert 0.0 < e <= 1e-4 * a["scale_v"]
  assert a["scale_v"] >= np.abs(a["rows"]).max() and a["scale_gx"] > 0.0 and a["scale_gs"] > 0.0


def test_spec_refusals():
  from cnf_ot_amd import _capi, utils
  ok = utils.stein_spec("imq", [0.5, 2.0], -0.25, [1.0, 3.0])
  assert (ok.kind, ok.n_terms, ok.beta) == (1, 2, -0.25) and list(ok.w)[:2] == [1.0, 3.0] and list(ok.bw)[:2] == [0.5, 2.0]
  assert utils.stein_spec("gaussian", [1.0]).kind == _capi.STEIN_KINDS["gaussian"] == 2
  bad = [dict(kind="laplace"), dict(bandwidths=[]), dict(bandwidths=[1.0] * 5), dict(bandwidths=[1.0, 2.0], weights=[1.0]),
         dict(bandwidths=[0.0]), dict(bandwidths=[-1.0]), dict(bandwidths=[float("inf")]), dict(bandwidths=[float("nan")]),
         dict(weights=[0.0]), dict(weights=[-1.0]), dict(weights=[float("inf")]), dict(weights=[float("nan")]),
         dict(beta=0.0), dict(beta=-1.0), dict(beta=0.5), dict(beta=float("nan")),
         dict(bandwidths=[1e-9]), dict(bandwidths=[1e-30]), dict(bandwidths=[1e25]),            # c^(2 beta - 6), c^2
         dict(kind="gaussian", bandwidths=[1e-7]), dict(kind="gaussian", bandwidths=[1e-30]),   # w / (8 h^6)
         dict(bandwidths=[1.0], weights=[3e38])]
  for kw in bad:
    with pytest.raises(ValueError):
      utils.stein_spec(**{"kind": "imq", "bandwidths": [1.0], **kw})
  assert utils.stein_spec("gaussian", [1.0], beta=5.0).beta == 0.0           # (the Gaussian kind does not read beta)


def test_shape_refusals():
  from cnf_ot_amd import utils
  utils.stein_check_shapes((64, 1 << 20, 14), (64, 1 << 20, 14))
  for shape in [(0, 8, 2), (65, 8, 2), (1, 1, 2), (1, (1 << 20) + 1, 2), (1, 8, 0), (1, 8, 15)]:
    with pytest.raises(ValueError):
      utils.stein_check_shapes(shape)
  with pytest.raises(ValueError):
    utils.stein_check_shapes((1, 8, 2), (1, 8, 3))
  # utils.ksd refuses before it looks for a device
  x = np.zeros((8, 2), dtype=np.float32)
  for args in [(np.zeros((8,)), x), (x, np.zeros((7, 2))), (np.zeros((1, 2)), np.zeros((1, 2))), (np.zeros((8, 15)), np.zeros((8, 15)))]:
    with pytest.raises(ValueError):
      utils.ksd(*args, bandwidths=[1.0])
  with pytest.raises(ValueError):
    utils.ksd(x + np.arange(8)[:, None], x, kind="imq", bandwidths=[1.0], beta=-2.0)


def test_loss_fn_refusals():
  from cnf_ot_amd import FlowConfig, FlowModel, applications as app
  from cnf_ot_amd.distributed import Shard
  from cnf_ot_amd.flows import DeviceRng
  model = FlowModel(FlowConfig(dim=2))
  tgt = app.GaussianMixtureTarget(np.zeros((1, 2)))
  call = lambda **kw: app.ksd_loss_fn(model, kw.pop("dim", 2), None, kw.pop("target", tgt), [0.5], kw.pop("rng", 1),
                                      kw.pop("batch", 64), **kw)
  with pytest.raises(ValueError, match="single rank"):
    call(shard=Shard(0, 2))
  with pytest.raises(ValueError, match="eager"):
    call(rng=DeviceRng.__new__(DeviceRng))
  with pytest.raises(ValueError, match="target"):
    call(target=3.0)
  for kw in [dict(batch=1), dict(dim=15), dict(kind="laplace"), dict(beta=0.25), dict(bandwidths=[0.0]), dict(weights=[-1.0] * 4),
             dict(bandwidths=[1.0, 2.0], weights=[1.0])]:
    with pytest.raises(ValueError):
      call(**kw)


def test_the_struct_is_the_headers():
  from cnf_ot_amd import _capi
  header = open(os.path.join(REPO, "include", "cnf_ot_amd.h")).read()
  body = re.search(r"typedef struct CnfSteinSpec \{(.*?)\} CnfSteinSpec;", header, re.S).group(1)
  fields = re.findall(r"\b(?:int32_t|float)\s+(\w+)", body)
  assert fields == [n for n, _ in _capi.CnfSteinSpec._fields_] == ["kind", "n_terms", "w", "bw", "beta"]
  assert ctypes.sizeof(_capi.CnfSteinSpec) == 8 + 2 * 4 * _capi.STEIN_MAX_TERMS + 4
  assert re.search(r"#define CNF_STEIN_MAX_TERMS 4\b", header) and _capi.STEIN_MAX_TERMS == 4
  assert re.search(r"CNF_STEIN_IMQ = 1, CNF_STEIN_GAUSSIAN = 2", header) and _capi.STEIN_KINDS == {"imq": 1, "gaussian": 2}
  for name in ("cnf_stein_workspace", "cnf_stein_splits", "cnf_stein"):
    assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header)


@pytest.mark.parametrize("scale", [None, 0.7])
def test_mixture_score_is_the_gradient_of_its_log_density(scale):
  from cnf_ot_amd import applications as app
  D = 3
  rng = np.random.default_rng(5)
  A = rng.standard_normal((D, D))
  cov = A @ A.T + 0.5 * np.eye(D)
  tgt = app.GaussianMixtureTarget(rng.standard_normal((3, D)) * 2.0, cov, [0.2, 0.5, 0.3])
  x = torch.from_numpy(rng.standard_normal((2, 7, D)) * 2.0).requires_grad_(True)
  v = 1.0 if scale is None else scale
  prec = torch.from_numpy(np.linalg.inv(cov * v))
  d = x[..., None, :] - torch.from_numpy(tgt.means)
  logp = torch.logsumexp(torch.from_numpy(tgt.log_weights) - 0.5 * torch.einsum("...a,ab,...b->...", d, prec, d), dim=-1)
  want, = torch.autograd.grad(logp.sum(), x, create_graph=True)
  got = tgt.score(x, scale)
  assert got.shape == x.shape and got.dtype == torch.float64
  assert float((got - want).detach().abs().max()) <= 1e-12 * float(want.detach().abs().max())
  # differentiable: its own vector-Jacobian product equals that of the autograd score
  g = torch.from_numpy(rng.standard_normal(tuple(x.shape)))
  a, = torch.autograd.grad(got, x, g, retain_graph=True)
  b, = torch.autograd.grad(want, x, g)
  assert float((a - b).abs().max()) <= 1e-11 * float(b.abs().max())
  with pytest.raises(ValueError):
    tgt.score(torch.zeros(4, D + 1))


def test_stationary_score_refusals():
  from cnf_ot_amd import applications as app
  x = np.zeros((8, 2), dtype=np.float32)
  quad = {"kind": "quadratic", "amplitudes": [0.5]}
  for kw in [dict(subtype="gradient"), dict(subtype="nongradient"), dict(subtype="lorenz"), dict(subtype="nope"),
             dict(sigma=0.0), dict(sigma=float("nan")), dict(a=float("inf")), dict(strength=float("nan")),
             dict(interaction={"kind": "gaussian", "amplitudes": [0.0]}), dict(interaction={"kind": "laplace"})]:
    args = {"a": 1.0, "sigma": 0.5, "subtype": "ou", "interaction": quad, "strength": 1.0, **kw}
    with pytest.raises(ValueError):
      app.mv_stationary_score(x, **args)
