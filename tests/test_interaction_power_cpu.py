"""CPU tests of the power kind of the interaction units (softened power laws and the log kernel): the spec and every
refusal, from each public entry point and from the C ABI with fake pointers -- so every one comes before a device is
touched -- and the float64 restatement (tests/interaction_power_ref.py) pinned against algebra to 1e-12: the quadratic
kind at pw = 2, eps = 0; central differences of W and of the force; the force's continuity through pw = 0; the log
kernel's virial sum.  The restatement of the particle system with the log kernel meets the closed form
applications.mv_log_second_moment, with the softening and Euler terms it computes itself, within the 5 standard errors
the GPU test uses (figures in the test's output: run with -s).
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interaction_power_ref as pr
import interaction_ref as ir
import interaction_vjp_ref as ivr

INF, NAN = float("inf"), float("nan")

# (python keyword arguments, the C spec's (amp, pw, eps)) of what every entry refuses; None: the C ABI has no such case
REFUSALS = [
  ({"amplitudes": [0.0]}, ((0.0,), (0.0,), 0.1)), ({"amplitudes": [INF]}, ((INF,), (0.0,), 0.1)),
  ({"amplitudes": [NAN]}, ((NAN,), (0.0,), 0.1)), ({"amplitudes": [1.0, 0.0], "exponents": [4.0, 1.0]}, ((1.0, 0.0), (4.0, 1.0), 0.1)),
  ({"exponents": [NAN]}, ((1.0,), (NAN,), 0.1)), ({"exponents": [INF]}, ((1.0,), (INF,), 0.1)),
  ({"exponents": [16.5]}, ((1.0,), (16.5,), 0.1)), ({"exponents": [-17.0]}, ((1.0,), (-17.0,), 0.1)),
  ({"bandwidths": -0.1}, ((1.0,), (0.0,), -0.1)), ({"bandwidths": INF}, ((1.0,), (0.0,), INF)),
  ({"bandwidths": NAN}, ((1.0,), (0.0,), NAN)), ({"bandwidths": 1e30, "exponents": [2.0]}, ((1.0,), (2.0,), 1e30)),
  ({"bandwidths": None}, ((1.0,), (0.0,), 0.0)), ({"bandwidths": 0.0, "exponents": [1.9]}, ((1.0,), (1.9,), 0.0)),
  ({"bandwidths": None, "exponents": [4.0, -1.0], "amplitudes": [1.0, 1.0]}, ((1.0, 1.0), (4.0, -1.0), 0.0)),
  ({"amplitudes": [1e30], "exponents": [-2.0], "bandwidths": 1e-3}, ((1e30,), (-2.0,), 1e-3)),      # amp eps^(p - 2)
  ({"amplitudes": [1e5], "exponents": [12.0], "bandwidths": 1e3}, ((1e5,), (12.0,), 1e3)),          # amp eps^p / p alone
  ({"amplitudes": [1e30], "exponents": [1e-10], "bandwidths": 1.0}, ((1e30,), (1e-10,), 1.0)),      # amp / p alone
  # a small softening length with a negative exponent: eps^(p - 2) leaves float64 itself
  ({"amplitudes": [1.0], "exponents": [-16.0], "bandwidths": 1e-20}, ((1.0,), (-16.0,), 1e-20)),
  ({"amplitudes": [1e-30], "exponents": [-14.0], "bandwidths": 1e-22}, ((1e-30,), (-14.0,), 1e-22)),
  ({"amplitudes": [1.0, 1.0], "exponents": [0.0, -16.0], "bandwidths": 1e-30}, ((1.0, 1.0), (0.0, -16.0), 1e-30)),
  ({"exponents": None}, None), ({"exponents": []}, ((), (), 0.1)), ({"exponents": [1.0] * 5, "amplitudes": [1.0] * 5}, None),
  ({"exponents": [1.0, 2.0]}, None), ({"bandwidths": [0.1, 0.2]}, None),
]
# accepted by cnf_interaction, refused by cnf_interaction_vjp: amp (p - 2) eps^(p - 4) alone leaves float32's range
HESSIAN_REFUSALS = [({"amplitudes": [1.0], "exponents": [-10.0], "bandwidths": 1e-3}, ((1.0,), (-10.0,), 1e-3)),
                    ({"amplitudes": [1.0], "exponents": [3.0], "bandwidths": None}, ((1.0,), (3.0,), 0.0))]
GOOD = dict(kind="power", amplitudes=[1.0], bandwidths=0.1, exponents=[0.0])


def _cspec(amp=(1.0, -1.0), pw=(4.0, 1.0), eps=0.05, kind=4, n_terms=None):
  from cnf_ot_amd import _capi
  s = _capi.CnfInteractionSpec()
  s.kind, s.n_terms = kind, len(pw) if n_terms is None else n_terms
  for i, v in enumerate(amp):
    s.amp[i] = v
  for i, v in enumerate(pw):
    s.pw[i] = v
  s.bw[0] = eps
  s.bw[1], s.bw[2], s.bw[3] = -7.0, NAN, 0.0       # (ignored by the power kind)
  return s


def test_the_spec():
  from cnf_ot_amd import _capi, interaction, utils
  assert _capi.INTERACTION_KINDS["power"] == 4 and 3 not in _capi.INTERACTION_KINDS.values()
  assert ctypes.sizeof(_capi.CnfInteractionSpec) == 8 + 3 * 4 * _capi.INTERACTION_MAX_TERMS
  assert [n for n, _ in _capi.CnfInteractionSpec._fields_] == ["kind", "n_terms", "amp", "bw", "pw"]
  s = utils.interaction_spec("power", [1.0, -1.0], 0.05, exponents=[4.0, 1.0])
  assert (s.kind, s.n_terms, list(s.amp)[:2], list(s.pw)[:2]) == (4, 2, [1.0, -1.0], [4.0, 1.0])
  assert s.bw[0] == float(np.float32(0.05))
  s = utils.interaction_spec("power", exponents=[2.0, 4.0, 16.0, 3.0])      # no softening: every exponent >= 2
  assert (s.n_terms, list(s.amp), list(s.pw), s.bw[0]) == (4, [1.0] * 4, [2.0, 4.0, 16.0, 3.0], 0.0)
  s = utils.interaction_spec("power", [-2.0], [0.1], exponents=[-1.0])     # Coulomb in dimension 3, repulsive
  assert (s.n_terms, s.amp[0], s.pw[0], s.bw[0]) == (1, -2.0, -1.0, float(np.float32(0.1)))
  interaction.interaction_vjp_check_spec(s)
  interaction.interaction_vjp_check_spec(utils.interaction_spec("power", exponents=[2.0, 4.0]))      # eps = 0: p = 2 and p >= 4
  for kw, _ in HESSIAN_REFUSALS:
    with pytest.raises(ValueError, match="Hessian"):
      interaction.interaction_vjp_check_spec(utils.interaction_spec(**dict(GOOD, **kw)))
  with pytest.raises(ValueError):
    utils.interaction_spec("coulomb", exponents=[-1.0])
  for kind in ("gaussian", "exponential", "quadratic"):
    with pytest.raises(ValueError, match="exponents"):
      utils.interaction_spec(kind, exponents=[1.0])
    assert utils.interaction_spec(kind).kind == _capi.INTERACTION_KINDS[kind]
    assert list(utils.interaction_spec(kind).pw) == [0.0] * 4


class _NoBackend:
  """A model that must not be asked for its backend"""
  def terms_backend(self, params, device=None):
    raise AssertionError("the backend was asked for")


def _entry_points(kw):
  import torch
  from cnf_ot_amd import applications as app, autograd, utils
  from cnf_ot_amd.distributed import Shard
  x = np.zeros((5, 3), dtype=np.float32)
  one = Shard(0, 1)
  first = [
    ("interaction_spec", lambda: utils.interaction_spec(**kw)),
    ("interaction_energy", lambda: utils.interaction_energy(x, **kw)),
    ("interaction_field", lambda: utils.interaction_field(x, x, **kw)),
    ("autograd.interaction_energy", lambda: autograd.interaction_energy(torch.zeros(5, 3), **kw)),
    ("interaction_loss_fn", lambda: app.interaction_loss_fn(_NoBackend(), 3, None, [0.5], 0, 96, shard=one, **kw)),
    ("ot_loss_fn", lambda: app.ot_loss_fn(_NoBackend(), 2, 1, 0.01, 4, "free", None, 0, 5000.0, 2048, interaction=(kw, 0.5),
                                          shard=one)),
    ("rwpo_loss_fn", lambda: app.rwpo_loss_fn(_NoBackend(), 2, 2, 10, 0.01, 0.01, 4, "double_well", 1, None, 0, 5000.0, 2048,
                                              interaction=(kw, 0.5), shard=one)),
    ("mv_reference_particles", lambda: app.mv_reference_particles(2, 0.5, 0.0, 0.5, "ou", kw, 2.0, [0.0, 0.1], n_particles=64,
                                                                   replicas=2, h=0.01)),
  ]
  second = [
    ("interaction_force_vjp", lambda: utils.interaction_force_vjp(x, x, **kw)),
    ("autograd.interaction_force", lambda: autograd.interaction_force(torch.zeros(5, 3), **kw)),
    ("fp_loss_fn", lambda: app.fp_loss_fn(_NoBackend(), 3, 1.0, 1.0, 0.5, 0.01, 0.01, 3, "ou", None, 0, 5000.0, 2048,
                                          interaction=(kw, 1.0), shard=one)),
  ]
  return first, second


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_python_entry_points_refuse_before_the_device(index):
  kw = dict(GOOD, **REFUSALS[index][0])
  first, second = _entry_points(kw)
  for name, call in first + second:
    with pytest.raises(ValueError):
      call()
      pytest.fail(f"{name} accepted {kw}")


def test_the_hessian_coefficient_is_the_vjp_entries_refusal():
  from cnf_ot_amd import utils
  for bad, _ in HESSIAN_REFUSALS:
    kw = dict(GOOD, **bad)
    utils.interaction_spec(**kw)                    # the value and the force have nothing against it
    for name, call in _entry_points(kw)[1]:
      with pytest.raises(ValueError):
        call()
        pytest.fail(f"{name} accepted {kw}")


def test_exponents_belong_to_the_power_kind_at_every_entry_point():
  for kind in ("gaussian", "exponential", "quadratic"):
    first, second = _entry_points(dict(kind=kind, exponents=[2.0]))
    for name, call in first + second:
      with pytest.raises(ValueError):
        call()
        pytest.fail(f"{name} accepted exponents with {kind}")


def test_the_solvers_section_carries_the_exponents():
  from cnf_ot_amd import solvers, utils
  ia = {"kind": "power", "strength": 2.0, "amplitudes": [1.0], "bandwidths": 0.1, "exponents": [0.0]}
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou", "a": 0.0},
                                          "interaction": ia})
  kw = solvers._interaction_kwargs(config)
  assert kw == {"kind": "power", "amplitudes": [1.0], "bandwidths": 0.1, "exponents": [0.0]}
  assert utils.interaction_spec(**kw).kind == 4
  assert "exponents" not in solvers._interaction_kwargs(solvers.load_config(overrides={"interaction": {"kind": "gaussian"}}))
  assert {"second_moment", "second_moment_exact"} <= set(solvers.MV_REFERENCE_KEYS)
  for bad in ({"exponents": [1.0]}, {"exponents": [NAN]}, {"bandwidths": -1.0}):      # eps = 0.1 and p = 1 is fine; with
    cfg = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2},          # bandwidths None it is not
                                         "fp": {"velocity_field_type": "ou"}, "interaction": dict(ia, **bad)})
    if bad == {"exponents": [1.0]}:
      cfg["interaction"]["bandwidths"] = None
    with pytest.raises(ValueError):
      solvers.evaluate_mv_reference(cfg, times=[0.0, 0.01], n_particles=64, replicas=2, h=0.01)


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  nb, vb, mb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
  assert lib.cnf_interaction_workspace(3, 300, 0, 10, 1, ctypes.byref(nb)) == _capi.CNF_OK
  assert lib.cnf_interaction_vjp_workspace(3, 300, 10, ctypes.byref(vb)) == _capi.CNF_OK
  assert lib.cnf_mv_particles_workspace(2, 300, 3, 4, ctypes.byref(mb)) == _capi.CNF_OK
  snap = (ctypes.c_int64 * 4)(0, 1, 5, 12)

  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  def pairs(spec, **kw):
    a = dict(S=3, N=300, D=10, wsb=nb.value, **kw)
    return lib.cnf_interaction(ctypes.byref(spec), a["S"], 4096, a["N"], None, 0, a["D"], 12288, 16384, 20480, 24576, a["wsb"],
                               None)

  def vjp(spec, **kw):
    a = dict(S=3, N=300, D=10, wsb=vb.value, **kw)
    return lib.cnf_interaction_vjp(ctypes.byref(spec), a["S"], 4096, 8192, a["N"], a["D"], 12288, 16384, a["wsb"], None)

  def particles(spec, **kw):
    a = dict(N=300, D=3, wsb=mb.value, **kw)
    return lib.cnf_mv_particles(ctypes.byref(spec), 1.5, 0, a["D"], 1.0, 0.5, 0.01, 12, 1.0, 7, 0, 2, a["N"], None, snap, 4, None,
                                4096, 8192, 12288, None, 20480, a["wsb"], None)

  entries = (("cnf_interaction", pairs), ("cnf_interaction_vjp", vjp), ("cnf_mv_particles", particles))
  for kw, c in REFUSALS:
    if c is None:
      continue
    for name, call in entries:
      assert call(_cspec(*c)) == INV, (name, kw)
  for bad in (_cspec(n_terms=0), _cspec(n_terms=5), _cspec(kind=3), _cspec(kind=5), _cspec(amp=(1.0, NAN)),
              _cspec(amp=(1.0,), pw=(0.0,), eps=0.1, n_terms=2)):                    # (the second term's amp is 0)
    for name, call in entries:
      assert call(bad) == INV, name
  for _, c in HESSIAN_REFUSALS:
    assert vjp(_cspec(*c)) == INV


# ---- the restatement against algebra ----------------------------------------------------------------------------------

SPECS = {"log": pr.spec([0.0], [1.0], 0.1), "coulomb3": pr.spec([-1.0], [-1.0], 0.1),
         "attractive-repulsive": pr.spec([4.0, 1.0], [1.0, -1.0], 0.05), "p2": pr.spec([2.0], [0.75], 0.0),
         "mixed/4": pr.spec([4.0, 1.0, 0.0, -1.0], [0.5, -1.0, 0.75, -0.25], 0.2)}


def test_p_2_without_softening_is_the_quadratic_restatement():
  x, q = ir.cloud(3, 70, 1).astype(np.float64), ir.cloud(3, 9, 2).astype(np.float64)
  sp, quad = SPECS["p2"], ir.spec("quadratic", [0.75])
  for qq in (None, q):
    a, b = pr.rows(x, sp, qq), ir.rows(x, quad, qq)
    for u, v in zip(a[:3], b[:3]):
      assert np.abs(np.asarray(u) - np.asarray(v)).max() <= 1e-12 * max(1.0, float(np.abs(np.asarray(v)).max()))
  g = ir.cloud(3, 70, 3).astype(np.float64)
  assert np.abs(pr.force_vjp(x, g, sp) - ivr.quadratic_closed_form(g, 0.75)).max() <= 1e-12
  k_max, tau, eta = pr.scales(x, sp)
  assert abs(k_max - ir.k_max(x, quad)) <= 1e-12 * k_max and abs(tau - ir.tau(x, quad)) <= 1e-12 * tau and abs(eta - 0.75) <= 1e-12


@pytest.mark.parametrize("name", list(SPECS))
def test_force_and_hessian_are_the_derivatives_of_w(name):
  sp = SPECS[name]
  rng = np.random.default_rng(5)
  D, h = 3, 1e-4
  d = rng.standard_normal((40, D)) * np.array([0.05, 0.5, 2.0, 4.0] * 10)[:, None]      # near and far pairs
  W = lambda v: pr.kernel(v[:, None, :], sp)[0][:, 0]
  F = lambda v: v * pr.kernel(v[:, None, :], sp)[1]
  v = rng.standard_normal((40, D))
  c1, c2 = pr.hessian_coefficients((d * d).sum(-1), sp)
  Hv = c1[:, None] * v + d * ((d * v).sum(-1) * c2)[:, None]
  u0 = np.maximum((d * d).sum(-1) + sp["eps"] ** 2, 1e-300)
  for e in range(D):
    step = np.zeros(D)
    step[e] = h
    # five-point central differences: error O(h^4) of the fifth derivative
    dW = (-W(d + 2 * step) + 8 * W(d + step) - 8 * W(d - step) + W(d - 2 * step)) / (12 * h)
    scale = np.maximum(1.0, np.abs(F(d)[:, e]))
    assert (np.abs(dW - F(d)[:, e]) <= 1e-9 * scale * np.maximum(1.0, 1.0 / u0 ** 3)).all(), name
  # the Hessian against differences of the force along v: a directional derivative
  t = 1e-4
  vn = v / np.linalg.norm(v, axis=1, keepdims=True)
  dF = (-F(d + 2 * t * vn) + 8 * F(d + t * vn) - 8 * F(d - t * vn) + F(d - 2 * t * vn)) / (12 * t)
  Hvn = c1[:, None] * vn + d * ((d * vn).sum(-1) * c2)[:, None]
  u = (d * d).sum(-1) + sp["eps"] ** 2
  assert (np.abs(dF - Hvn) <= 1e-8 * np.maximum(1.0, np.abs(Hvn).max(1, keepdims=True)) * np.maximum(1.0, 1.0 / u ** 3)[:, None]).all()
  assert np.isfinite(Hv).all()
  # and the closed forms to 1e-12 where they are algebra: W' r = w r^2, the eigenvalue along d is c1 + c2 r^2
  r2 = (d * d).sum(-1)
  want_w = sum(a * u ** (p / 2.0 - 1.0) for a, p in zip(sp["amp"], sp["pw"]))
  want_along = sum(a * u ** (p / 2.0 - 2.0) * (u + (p - 2.0) * r2) for a, p in zip(sp["amp"], sp["pw"]))
  assert np.abs(c1 - want_w).max() <= 1e-12 * np.abs(want_w).max()
  assert np.abs(c1 + c2 * r2 - want_along).max() <= 1e-12 * np.abs(want_along).max()


def test_the_force_is_continuous_through_the_log_kernel():
  d = np.random.default_rng(6).standard_normal((30, 1, 2))
  w0 = pr.kernel(d, pr.spec([0.0], [1.5], 0.1))[1]
  W0 = pr.kernel(d, pr.spec([0.0], [1.5], 0.1))[0]
  for p in (1e-3, 1e-6, 1e-9):
    for s in (p, -p):
      sp = pr.spec([s], [1.5], 0.1)
      ps = sp["pw"][0]                                    # (the float32 rounding the spec carries)
      W, w = pr.kernel(d, sp)
      # w_p / w_0 = u^(p / 2): |w_p - w_0| <= |w_0| (exp(|p ln u| / 2) - 1)
      u = (d * d).sum(-1) + sp["eps"] ** 2
      assert (np.abs(w - w0) <= np.abs(w0) * np.expm1(np.abs(ps * np.log(u)) / 2.0) + 1e-14 * np.abs(w0)).all()      # (+ both weights' roundings)
      # and W_p - amp / p -> W_0: u^(p/2) / p - 1 / p = ln(u) / 2 + O(p ln(u)^2 / 8)
      assert (np.abs((W - 1.5 / ps) - W0) <= 1.5 * np.abs(ps) * np.log(u) ** 2 / 8.0 * 1.01 + 1e-15 * 1.5 / abs(ps)).all()
  assert np.abs(pr.kernel(d, pr.spec([1e-9], [1.5], 0.1))[1] - w0).max() <= 1e-8 * np.abs(w0).max()


@pytest.mark.parametrize("D", [1, 2, 3, 7])
def test_the_virial_sum_of_the_log_kernel(D):
  """sum_i x_i . f_i = amp N / 2 with f_i the mean over the N - 1 others: every dimension, every N"""
  for N in (2, 3, 50):
    x = ir.cloud(D, N, 10 + N).astype(np.float64)
    sp = {"kind": "power", "amp": [1.25], "pw": [0.0], "eps": 0.0}        # (the restatement takes eps = 0: no pair coincides)
    assert abs(pr.virial_sum(x, sp) - 1.25 * N / 2.0) <= 1e-12 * N
    # softened: every pair's 1 becomes d^2 / (d^2 + eps^2)
    soft = dict(sp, eps=0.3)
    diff = x[:, None, :] - x[None, :, :]
    d2 = (diff * diff).sum(-1)[~np.eye(N, dtype=bool)]
    assert abs(pr.virial_sum(x, soft) - 1.25 * N / 2.0 * float((d2 / (d2 + 0.09)).mean())) <= 1e-12 * N


def test_the_particle_restatement_meets_the_closed_form():
  """The GPU test's check (test_gpu_mv_particles_power.py), on the restatement alone with NumPy's normals"""
  from cnf_ot_amd import applications as app
  D, R, N, steps, h, sigma, kappa, amp, eps, var0 = 2, 8, 128, 200, 0.005, 0.25, 3.0, -1.0, 0.1, 1.0
  sp = pr.spec([0.0], [amp], eps)
  z = np.random.default_rng(11).standard_normal((R, N, steps + 1, D))
  m2, expected, resid = pr.log_second_moment_increments(z, sigma, h, var0, kappa, sp, steps)
  T = steps * h
  closed = app.mv_log_second_moment(T, D, sigma, kappa, amp, 0.0)
  assert closed == (2.0 * D * sigma - kappa * amp) * T and app.mv_log_second_moment(0.0, D, sigma, kappa, amp, 1.5) == 1.5
  got = float((m2[-1] - m2[0]).mean())
  corrections = float(expected.mean()) - closed              # the softening (< 0 here: less repulsion) and Euler (> 0) terms
  se = float(resid.std(ddof=1)) / math.sqrt(R * N)
  print(f"\n[log kernel, restatement, D={D} R={R} N={N} {steps} steps] mean |x|^2 grew by {got:.5f}; closed form {closed:.5f} + "
        f"softening and Euler terms {corrections:+.5f}; standard error {se:.5f}: z = {(got - closed - corrections) / se:+.2f} "
        f"(without the force: {2.0 * D * sigma * T:.3f})")
  assert abs(got - (closed + corrections)) <= 5.0 * se
  assert abs(corrections) < 0.1 * abs(closed) and 5.0 * se < 0.25 * abs(kappa * amp * T)      # the check can see the force
