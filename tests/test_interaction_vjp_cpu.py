"""The interacting Fokker-Planck training term without a GPU: the float64 restatement of the force's vector-Jacobian
product (tests/interaction_vjp_ref.py) against central differences of interaction_ref's force and against its own
identities, the restated epilogue with a force against step_kernels_ref and central differences, the host-side argument
checks of cnf_interaction_vjp and cnf_score_residual_force through the C ABI (no device is touched), the Python entry
points' refusals, which come before any device work, and the config section's `role`.

Central differences use h = 1e-5 in float64: truncation h^2 |f'''| / 6 and rounding 2^-53 |f| / h are both below 1e-9
of the scale max(1, max |xbar|) for these kernels (bandwidths >= 0.5, amplitudes <= 1), so 1e-7 of that scale is asked.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interaction_ref as ir
import interaction_vjp_ref as ivr
import step_kernels_ref as sk

SPECS = {"gaussian": ir.spec("gaussian", [1.0, -0.5], [0.75, 1.5]),
         "exponential": ir.spec("exponential", [1.0, -0.5], [0.5, 2.0]),
         "quadratic": ir.spec("quadratic", [0.75])}


def _objective(x, g, sp):
  return float((g * ir.force(x, sp)).sum())


@pytest.mark.parametrize("N", [2, 7, 33])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("kind", list(SPECS))
def test_restatement_against_central_differences_of_the_force(kind, D, N):
  sp, h = SPECS[kind], 1e-5
  x = ir.cloud(D, N, seed=10 * D + N).astype(np.float64)
  g = np.random.default_rng(5 + N).standard_normal((N, D))
  got = ivr.force_vjp(x, g, sp)
  want = np.empty_like(x)
  for i in range(N):
    for d in range(D):
      xp, xm = x.copy(), x.copy()
      xp[i, d] += h
      xm[i, d] -= h
      want[i, d] = (_objective(xp, g, sp) - _objective(xm, g, sp)) / (2.0 * h)
  err = float(np.abs(got - want).max())
  print(f"[force vjp restatement {kind} D={D} N={N}] error {err:.2e} at |xbar| {np.abs(want).max():.2e}")
  assert err <= 1e-7 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("kind", list(SPECS))
def test_identities_of_the_restatement(kind):
  sp, D, N = SPECS[kind], 3, 41
  x = ir.cloud(D, N, seed=3).astype(np.float64)
  rng = np.random.default_rng(4)
  g, g2 = rng.standard_normal((N, D)), rng.standard_normal((N, D))
  a, b = ivr.force_vjp(x, g, sp), ivr.force_vjp(x, g2, sp)
  scale = float(np.abs(a).max())
  assert np.abs(a.sum(0)).max() <= 1e-13 * N * scale                       # translations leave the force alone
  assert abs(float((g2 * a).sum()) - float((g * b).sum())) <= 1e-13 * N * D * scale * float(np.abs(g2).max())
  assert np.abs(ivr.force_vjp(x, np.ones((N, D)) * [1.0, -2.0, 3.0], sp)).max() == 0.0      # a constant adjoint
  if kind == "quadratic":
    assert np.abs(a - ivr.quadratic_closed_form(g, sp["amp"][0])).max() <= 1e-13 * scale
  assert ivr.hessian_norm(x, sp) > 0.0


def test_a_duplicated_point():
  """Two coincident points: the pair's Hessian is c1(0) I for the Gaussian kind (c2 is multiplied by d = 0) and 0 for
  the exponential kind, whose force is 0 there by rule"""
  x = np.array([[0.25, -1.0], [0.25, -1.0]])
  g = np.array([[1.0, 2.0], [-0.5, 0.25]])
  sp = SPECS["gaussian"]
  c1 = sum(-a / (b * b) for a, b in zip(sp["amp"], sp["bw"]))
  got = ivr.force_vjp(x, g, sp)
  assert np.allclose(got[0], c1 * (g[0] - g[1]), rtol=1e-15, atol=0.0) and np.allclose(got[1], -got[0], rtol=1e-15, atol=0.0)
  assert not ivr.force_vjp(x, g, SPECS["exponential"]).any()
  # beside a third point: the duplicates' pair adds exactly that to what the third point gives
  x3 = np.concatenate([x, [[1.0, 0.5]]])
  g3 = np.concatenate([g, [[0.0, -1.0]]])
  far = ivr.force_vjp(x3[[0, 2]], g3[[0, 2]], sp)[0]          # (N - 1 = 1 there, 2 here)
  assert np.allclose(ivr.force_vjp(x3, g3, sp)[0], 0.5 * (far + c1 * (g[0] - g[1])), rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("D,drift", [(2, None), (2, "ou"), (2, "gradient"), (2, "nongradient"), (3, "lorenz")])
def test_the_epilogue_with_a_force(D, drift):
  n, count, dt, coef, a, c, strength, h = 24, 7, 0.01, 0.7, 1.3, 0.37, 1.7, 1e-5
  rng = np.random.default_rng(8 + D)
  r, score, force = 1.5 * rng.standard_normal((3 * n, D)), rng.standard_normal((n, D)), rng.standard_normal((n, D))
  base = sk.score_residual_ref(r, score, n, count, D, dt, coef, drift, a, c)
  zero = ivr.score_residual_force_ref(r, score, force, 0.0, n, count, D, dt, coef, drift, a, c)
  for got, want in zip(zero[:3], base):
    assert np.array_equal(got, want)
  assert not zero[3].any()
  sums, rbar, sbar, fbar = ivr.score_residual_force_ref(r, score, force, strength, n, count, D, dt, coef, drift, a, c)
  loss = lambda rr, ss, ff: c * float(ivr.score_residual_force_ref(rr, ss, ff, strength, n, count, D, dt, coef, drift, a, c)[0].sum())
  for name, arr, bar, pos in (("force", force, fbar, 2), ("score", score, sbar, 1), ("r", r, rbar, 0)):
    want = np.empty_like(arr)
    for idx in np.ndindex(*arr.shape):
      p, m = arr.copy(), arr.copy()
      p[idx] += h
      m[idx] -= h
      args = [r, score, force]
      lp = loss(*[p if k == pos else v for k, v in enumerate(args)])
      lm = loss(*[m if k == pos else v for k, v in enumerate(args)])
      want[idx] = (lp - lm) / (2.0 * h)
    err = float(np.abs(bar - want).max())
    print(f"[epilogue with force D={D} {drift}] {name}bar error {err:.2e} at {np.abs(want).max():.2e}")
    assert err <= 1e-6 * max(1.0, float(np.abs(want).max()))


def _cspec(kind=0, n_terms=2, amp=(1.0, -0.5), bw=(0.5, 2.0)):
  from cnf_ot_amd import _capi
  s = _capi.CnfInteractionSpec()
  s.kind, s.n_terms = kind, n_terms
  for i, a in enumerate(amp):
    s.amp[i] = a
  for i, b in enumerate(bw):
    s.bw[i] = b
  return s


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_interaction_vjp_workspace(3, 300, 10, ctypes.byref(nbytes)) == _capi.CNF_OK
  assert nbytes.value == 8 * 3 * lib.cnf_interaction_splits(3, 300, 0, 10) * 300 * 10
  other = ctypes.c_int64(0)
  for bad in ((0, 300, 10), (65, 300, 10), (3, 1, 10), (3, 300, 0), (3, 300, 15), (3, (1 << 20) + 1, 2)):
    assert lib.cnf_interaction_vjp_workspace(*bad, ctypes.byref(other)) == INV, bad
  assert lib.cnf_interaction_vjp_workspace(3, 300, 10, None) == INV
  # monotone in each argument: S P N D doubles, P = cnf_interaction_splits.  In D everywhere; in S and N while every
  # tile of 64 columns is a split of its own (S x row groups x tiles <= 2048 workgroups, here N <= 1100 for up to 3 sets:
  # beyond that the split count follows the workgroup target down as the row groups grow)
  size = lambda S, N, D: (lib.cnf_interaction_vjp_workspace(S, N, D, ctypes.byref(other)), other.value)[1]
  for S, N, D in ((1, 2, 1), (3, 300, 10), (32, 4096, 2), (9, 32768, 10), (64, 1 << 20, 13)):
    assert size(S, N, D) == 8 * S * lib.cnf_interaction_splits(S, N, 0, D) * N * D
    assert size(S, N, D + 1) > size(S, N, D)
  for D in (1, 14):
    for S in (1, 2, 3):
      sizes = [size(S, N, D) for N in range(2, 1101)]
      assert all(b > a for a, b in zip(sizes, sizes[1:]))
    for N in (2, 64, 65, 700, 1100):
      assert size(1, N, D) < size(2, N, D) < size(3, N, D)

  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  good = dict(spec=_cspec(), S=3, x=4096, g=8192, N=300, D=10, xbar=12288, ws=16384, wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_interaction_vjp(None if a["spec"] is None else ctypes.byref(a["spec"]), a["S"], a["x"], a["g"], a["N"],
                                   a["D"], a["xbar"], a["ws"], a["wsb"], None)

  inf, nan = float("inf"), float("nan")
  for bad in ({"spec": None}, {"x": None}, {"g": None}, {"xbar": None}, {"ws": None}, {"D": 0}, {"D": 15}, {"N": 1},
              {"N": (1 << 20) + 1}, {"S": 0}, {"S": 65},
              {"spec": _cspec(kind=3)}, {"spec": _cspec(kind=-1)}, {"spec": _cspec(n_terms=0)}, {"spec": _cspec(n_terms=5)},
              {"spec": _cspec(amp=(1.0, 0.0))}, {"spec": _cspec(amp=(1.0, inf))}, {"spec": _cspec(amp=(nan, 1.0))},
              {"spec": _cspec(bw=(1.0, 0.0))}, {"spec": _cspec(bw=(1.0, -2.0))}, {"spec": _cspec(bw=(inf, 1.0))},
              {"spec": _cspec(bw=(nan, 1.0))}, {"spec": _cspec(bw=(1e-30, 1.0))}, {"spec": _cspec(kind=1, bw=(1e-30, 1.0))},
              {"spec": _cspec(amp=(1e30, 1.0), bw=(1e-6, 1.0))}, {"spec": _cspec(kind=2, amp=(0.0,))},
              {"spec": _cspec(kind=2, amp=(nan,))},
              {"spec": _cspec(amp=(1.0, 1.0), bw=(1e-10, 1.0))},             # amp / bw^2 fits, amp / bw^4 does not
              {"spec": _cspec(kind=1, amp=(1.0, 1.0), bw=(1e-20, 1.0))},     # amp / bw fits, amp / bw^2 does not
              {"wsb": nbytes.value - 8}, {"wsb": 0}):
    assert call(**bad) == INV, bad

  f32, f64 = np.full(64, 7.25, np.float32), np.full(8, 7.25, np.float64)
  p, d = f32.ctypes.data, f64.ctypes.data

  def score(r=p, s=p, f=p, n=4, count=2, D=2, dt=0.1, drift=_capi.DRIFTS["ou"], sums=d, rb=p, sb=p, fb=p):
    return lib.cnf_score_residual_force(r, s, f, 0.8, n, count, D, dt, 0.5, drift, 1.0, 0.37, sums, rb, sb, fb, None)

  bad = {"r=NULL": score(r=None), "score=NULL": score(s=None), "force=NULL": score(f=None), "sums=NULL": score(sums=None),
         "n<0": score(n=-1), "count<1": score(count=0), "D<1": score(D=0), "dt=0": score(dt=0.0), "dt<0": score(dt=-0.1),
         "rbar alone": score(sb=None, fb=None), "sbar alone": score(rb=None, fb=None), "fbar alone": score(rb=None, sb=None),
         "fbar missing": score(fb=None), "rbar missing": score(rb=None), "sbar missing": score(sb=None),
         "drift=7": score(drift=7), "drift=-2": score(drift=-2), "smile at D=3": score(D=3, drift=_capi.DRIFTS["smile"]),
         "nongradient at D=3": score(D=3, drift=_capi.DRIFTS["nongradient"]),
         "lorenz at D=2": score(D=2, drift=_capi.DRIFTS["lorenz"])}
  wrong = {k: v for k, v in bad.items() if v != INV}
  assert not wrong, wrong
  assert (f32 == 7.25).all() and (f64 == 7.25).all()


class _Untouchable:
  """A terms backend that raises if it is touched"""
  def __getattr__(self, name):
    raise AssertionError(f"the backend was touched: {name}")


class _NoBackend:
  """A model that must not be asked for its backend"""
  def terms_backend(self, params, device=None):
    raise AssertionError("the backend was asked for")


class _NoEngine:
  """A model whose terms backend is not the HIP engine, and raises if it is touched"""
  def terms_backend(self, params, device=None):
    return _Untouchable()


def test_python_entry_points_refuse_before_the_device():
  import torch
  from cnf_ot_amd import applications as app, autograd, utils
  from cnf_ot_amd.distributed import Shard
  from cnf_ot_amd.flows import DeviceRng
  x = np.zeros((5, 3), dtype=np.float32)
  inf, nan = float("inf"), float("nan")
  bad_specs = ({"kind": "coulomb"}, {"amplitudes": [1.0] * 5, "bandwidths": [1.0] * 5}, {"amplitudes": [], "bandwidths": []},
               {"amplitudes": [1.0, 2.0], "bandwidths": [1.0]}, {"amplitudes": [0.0]}, {"amplitudes": [inf]},
               {"amplitudes": [nan]}, {"bandwidths": [0.0]}, {"bandwidths": [-1.0]}, {"bandwidths": [inf]},
               {"bandwidths": [nan]}, {"bandwidths": [1e-30]}, {"amplitudes": [1e30], "bandwidths": [1e-6]},
               {"bandwidths": [1e-10]}, {"kind": "exponential", "bandwidths": [1e-20]},
               {"kind": "exponential", "bandwidths": [1e-30]}, {"kind": "quadratic", "amplitudes": [0.0]},
               {"kind": "quadratic", "amplitudes": [1.0, 2.0]}, {"kind": "quadratic", "amplitudes": [nan]})
  fp = lambda model=None, dim=3, sub="ou", rng=0, batch=2048, **kw: app.fp_loss_fn(
      model if model is not None else _NoBackend(), dim, 1.0, 1.0, 0.5, 0.01, 0.01, 3, sub, None, rng, 5000.0, batch, **kw)
  for bad in bad_specs:
    kw = dict(dict(kind="gaussian", amplitudes=[1.0], bandwidths=[1.0]), **bad)
    for call in (lambda: utils.interaction_force_vjp(x, x, **kw), lambda: autograd.interaction_force(torch.zeros(5, 3), **kw),
                 lambda: fp(interaction=(kw, 1.0), shard=Shard(0, 1))):
      with pytest.raises(ValueError):
        call()
  for bx, bg in ((x[:1], x[:1]), (np.zeros(5), np.zeros(5)), (np.zeros((0, 5, 3)), np.zeros((0, 5, 3))), (np.zeros((5, 15)),) * 2,
                 (x, x[:4]), (x, np.zeros((5, 2))), (x, np.zeros((2, 5, 3))), (x, np.zeros(15))):
    with pytest.raises(ValueError):
      utils.interaction_force_vjp(bx, bg, "quadratic")
  with pytest.raises(ValueError):
    autograd.interaction_force(torch.zeros(1, 3), "quadratic")
  # fp_loss_fn(interaction=...): a captured step's rng, world > 1, sub < 2, a strength that is not finite, a drift that is
  # not defined at the dimension -- each before the backend is asked for -- and a backend that is not the HIP engine
  given = ({"kind": "quadratic"}, 0.5)
  rng_dev = DeviceRng.__new__(DeviceRng)      # (no device behind it: only its type is read)
  with pytest.raises(ValueError, match="eager update only"):
    fp(rng=rng_dev, interaction=given, shard=Shard(0, 1))
  with pytest.raises(ValueError, match="all-gather"):
    fp(interaction=given, shard=Shard(0, 2))
  with pytest.raises(ValueError, match="batch_size // 32"):
    fp(batch=63, interaction=given, shard=Shard(0, 1))
  for s in (inf, nan):
    with pytest.raises(ValueError, match="strength"):
      fp(interaction=({"kind": "quadratic"}, s), shard=Shard(0, 1))
  with pytest.raises(ValueError):
    fp(sub="gradient", interaction=given, shard=Shard(0, 1))          # (dim 3)
  with pytest.raises(ValueError):
    fp(sub="whirl", interaction=given, shard=Shard(0, 1))
  with pytest.raises(ValueError, match="HIP engine"):
    fp(model=_NoEngine(), interaction=given, shard=Shard(0, 1))


def test_bind_loss_reads_the_role():
  from cnf_ot_amd import solvers
  ia = {"kind": "gaussian", "strength": 2.0, "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}
  cfg = lambda _type, **extra: solvers.load_config(overrides={"interaction": dict(ia, **extra), "general": {"type": _type}})
  assert "role" not in solvers.DEFAULT_CONFIG["interaction"]
  fn = solvers.bind_loss(cfg("fp", role="drift"), None)
  kw, strength = fn.keywords["interaction"]
  assert strength == 2.0 and kw == {"kind": "gaussian", "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}
  assert "interaction" not in solvers.bind_loss(solvers.load_config(overrides={"general": {"type": "fp"}}), None).keywords
  # (kind "none": the role is not read)
  assert "interaction" not in solvers.bind_loss(
      solvers.load_config(overrides={"general": {"type": "fp"}, "interaction": {"role": "drift"}}), None).keywords
  for extra in ({}, {"role": "cost"}):
    with pytest.raises(ValueError, match="fp_loss_fn") as exc:
      solvers.bind_loss(cfg("fp", **extra), None)
    assert "role: drift" in str(exc.value)
    for _type in ("ot", "rwpo"):
      assert solvers.bind_loss(cfg(_type, **extra), None).keywords["interaction"] == (kw, 2.0)
  for _type in ("ot", "rwpo"):
    with pytest.raises(ValueError, match="drift"):
      solvers.bind_loss(cfg(_type, role="drift"), None)
  for _type in ("fp", "ot", "rwpo"):
    with pytest.raises(ValueError, match="role"):
      solvers.bind_loss(cfg(_type, role="force"), None)
  with pytest.raises(ValueError, match="eager update only"):
    solvers.train(cfg("fp", role="drift"), epochs=1, capture=True)


def test_the_command_line_and_the_evaluation_refuse_early():
  from cnf_ot_amd import solvers
  assert solvers._parse(["--mv-path"]).mv_path and not solvers._parse([]).mv_path
  ia = {"kind": "quadratic", "strength": 2.0, "amplitudes": [1.0], "role": "drift"}
  fp = {"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}}
  with pytest.raises(ValueError, match="--mv-path"):      # (the checked-in default: rwpo, kind "none")
    solvers.main(solvers.load_config(), mv_path=True)
  with pytest.raises(ValueError, match="--mv-path"):
    solvers.main(solvers.load_config(overrides=dict(fp, interaction=dict(ia, role="cost"))), mv_path=True)
  good = solvers.load_config(overrides=dict(fp, interaction=ia))
  for kw in ({"n": 1}, {"n": (1 << 20) + 1}, {"n_particles": 7}, {"replicas": 1}, {"times": [0.00037]}):
    with pytest.raises(ValueError):
      solvers.evaluate_mv_path(good, None, None, **kw)
  with pytest.raises(ValueError):
    solvers.evaluate_mv_path(solvers.load_config(overrides=fp), None, None)                       # kind "none"
  with pytest.raises(ValueError):
    solvers.evaluate_mv_path(solvers.load_config(overrides={"interaction": ia}), None, None)      # rwpo
  assert "fp_loss_fn" in solvers.evaluate_mv_reference.__doc__ and "no interacting training term" not in solvers.evaluate_mv_reference.__doc__
