"""CPU tests of the interacting particle reference (cnf_mv_particles / applications.mv_reference_particles /
solvers.evaluate_mv_reference): the float64 restatement (tests/mv_particles_f64.py) against independent algebra for the
drift ou with the quadratic kernel on given normals, the closed form of the mean-field limit against a fine float64
integration of its ODE, and every refusal of the C ABI (through the loaded library) and of the Python layer -- each
before any device work: this file runs without a GPU.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp_particles_f64 as fp
import interaction_ref as ir
import mv_particles_f64 as mv


def test_restatement_against_the_linear_algebra_of_ou_with_the_quadratic_kernel():
  R, N, D, steps = 2, 37, 3, 9
  a, sigma, h, var0, kappa, amp = 0.75, 0.4, 0.01, 1.3, 1.5, 0.8
  sp = ir.spec("quadratic", [amp])
  # normals that float32 holds exactly, and a start that it holds exactly too: the rounding of the positions the force
  # is formed on is then the only float32 effect, and it is below the 1e-12 asked for only at the start; so the algebra
  # is checked with the restatement's force on UNROUNDED positions (force=...), and the rounding's size separately
  z = np.random.default_rng(3).standard_normal((R, N, steps + 1, D)).astype(np.float32).astype(np.float64)
  exact_force = lambda x, s: ir.rows(x, s)[1:3]
  pos, _ = mv.integrate(z, "ou", a, sigma, h, var0, kappa, sp, range(steps + 1), force=exact_force)
  sdn = math.sqrt(2.0 * sigma * h)
  c = 1.0 - h * (a + kappa * amp * N / (N - 1.0))
  for r in range(R):
    G = ir.rows(pos[0, r], sp)[1]
    want = amp * N / (N - 1.0) * (pos[0, r] - pos[0, r].mean(0))
    print(f"[replica {r}] pair force against amp N / (N - 1) (x - mean): {np.abs(G - want).max():.2e}")
    assert np.abs(G - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
    for k in range(steps):
      x, xn, zk = pos[k, r], pos[k + 1, r], z[r, :, k + 1]
      mean_err = np.abs(xn.mean(0) - ((1.0 - h * a) * x.mean(0) + sdn * zk.mean(0))).max()
      dev_err = np.abs((xn - xn.mean(0)) - (c * (x - x.mean(0)) + sdn * (zk - zk.mean(0)))).max()
      assert mean_err <= 1e-12 and dev_err <= 1e-12, (r, k, mean_err, dev_err)
  # the force on the rounded positions (the restatement's default) differs by the rounding of x alone: amp N / (N - 1)
  # times 2^-24 |x| per coordinate, twice for the mean's share
  G32 = mv.force_f64(pos[3, 0], sp)[0]
  assert np.abs(G32 - ir.rows(pos[3, 0], sp)[1]).max() <= 2.0 * amp * N / (N - 1.0) * 2.0 ** -24 * np.abs(pos[3, 0]).max()


@pytest.mark.parametrize("subtype,D", [("ou", 1), ("gradient", 2), ("lorenz", 3), ("ou", 5)])
def test_restatement_without_the_force_is_the_fp_restatement(subtype, D):
  R, N, steps, snaps = 2, 19, 7, (0, 1, 4, 7)
  z = np.random.default_rng(5).standard_normal((R, N, steps + 1, D))
  sp = ir.spec("gaussian", [1.0, -0.5], [0.7, 1.9])
  pos, wsum = mv.integrate(z, subtype, 1.0, 0.5, 0.01, 1.2, 0.0, sp, snaps)
  for r in range(R):
    assert np.array_equal(pos[:, r], fp.integrate(z[r], subtype, 1.0, 0.5, 0.01, 1.2, snaps))
    for s in range(len(snaps)):
      assert wsum[s, r] == ir.sums(mv.rounded(pos[s, r]), sp)
  # the float32 composition of the force is the same force to float32's accuracy, its energy sum too
  G, t = mv.force_f64(pos[1, 0], sp)
  G32, t32 = mv.force_f32(pos[1, 0], sp)
  tau = ir.tau(mv.rounded(pos[1, 0]), sp)
  assert np.abs(G32 - G).max() <= 4 * mv.EPS32 * tau and abs(t32 - t) <= 4 * mv.EPS32 * 1.5 * N * (N - 1)


def test_the_replica_normals_follow_the_fp_stream_layout():
  R, N, steps, D = 2, 5, 3, 3
  stride = fp.stream_stride(steps, D)
  flat = np.arange(R * N * stride, dtype=np.float64)
  z = mv.replica_normals(flat, R, N, steps, D)
  assert z.shape == (R, N, steps + 1, D)
  assert z[1, 2, 0, 0] == (N + 2) * stride and z[1, 2, 3, 1] == (N + 2) * stride + 3 * D + 1


@pytest.mark.parametrize("a,strength,amp", [(1.0, 2.0, 1.0), (0.5, 4.0, 0.5), (1.0, -0.5, 1.0), (1.0, -1.0, 1.0),
                                            (0.5, -1.0, 1.0)])
def test_the_quadratic_ou_variance_solves_its_ode(a, strength, amp):
  from cnf_ot_amd import applications as app
  sigma, var0, T, n = 0.5, 1.5, 0.8, 20000
  lam = a + strength * amp
  f = lambda v: -2.0 * lam * v + 2.0 * sigma
  v, dt = var0, T / n
  for k in range(n + 1):
    if k in (0, n // 4, n):
      got = app.mv_quadratic_ou_variance(k * dt, a, sigma, strength, amp, var0)
      assert abs(got - v) <= 1e-10 * max(1.0, abs(v)), (k, got, v)
    k1 = f(v); k2 = f(v + 0.5 * dt * k1); k3 = f(v + 0.5 * dt * k2); k4 = f(v + dt * k3)      # RK4: error (lam dt)^4
    v += dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
  # without the interaction it is the existing closed form
  assert app.mv_quadratic_ou_variance(0.3, a, sigma, 0.0, amp, var0) == pytest.approx(app.ou_variance(0.3, a, var0, sigma),
                                                                                   rel=1e-14)


def _spec(kind=0, n_terms=2, amp=(1.0, -0.5), bw=(0.5, 2.0)):
  from cnf_ot_amd import _capi
  s = _capi.CnfInteractionSpec()
  s.kind, s.n_terms = kind, n_terms
  for i, v in enumerate(amp):
    s.amp[i] = v
  for i, v in enumerate(bw):
    s.bw[i] = v
  return s


def test_the_c_abi_refuses_before_the_device():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  R, N, D, S = 2, 300, 3, 4
  nbytes, pair = ctypes.c_int64(0), ctypes.c_int64(0)
  assert lib.cnf_mv_particles_workspace(R, N, D, S, ctypes.byref(nbytes)) == _capi.CNF_OK
  assert lib.cnf_interaction_workspace(R, N, 0, D, 1, ctypes.byref(pair)) == _capi.CNF_OK
  chunks, K = 2, 3 + D + D * D
  assert nbytes.value == pair.value + 8 * S * R * K * chunks + 4 * R * N * D       # pair partials, chunk partials, mirror
  assert nbytes.value % 8 == 0
  odd = ctypes.c_int64(0)
  assert lib.cnf_mv_particles_workspace(1, 3, 1, 1, ctypes.byref(odd)) == _capi.CNF_OK and odd.value % 8 == 0
  for bad in ((0, N, D, S), (65, N, D, S), (R, 1, D, S), (R, (1 << 20) + 1, D, S), (R, N, 0, S), (R, N, 15, S),
              (R, N, D, 0), (R, N, D, 65)):
    assert lib.cnf_mv_particles_workspace(*bad, ctypes.byref(odd)) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_mv_particles_workspace(R, N, D, S, None) == _capi.CNF_ERR_INVALID

  snap = (ctypes.c_int64 * 4)(0, 1, 5, 12)
  grid = _capi.CnfFieldGrid(-1.5, -1.0, 0.5, 0.5, 7, 5, 0, 1, -1, 1, None, None)
  # (fake non-NULL pointers: every refusal comes before anything is enqueued or dereferenced on the device)
  good = dict(spec=_spec(), kappa=1.5, drift=0, D=D, a=1.0, sigma=0.5, h=0.01, n_steps=12, var0=1.0, seed=7, first=0,
              R=R, N=N, x0=None, snap=snap, S=S, grid=grid, state=4096, pos=8192, sums=12288, hist=16384, ws=20480,
              wsb=nbytes.value)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_mv_particles(None if a["spec"] is None else ctypes.byref(a["spec"]), a["kappa"], a["drift"], a["D"],
                                a["a"], a["sigma"], a["h"], a["n_steps"], a["var0"], a["seed"], a["first"], a["R"],
                                a["N"], a["x0"], a["snap"], a["S"], None if a["grid"] is None else ctypes.byref(a["grid"]),
                                a["state"], a["pos"], a["sums"], a["hist"], a["ws"], a["wsb"], None)

  inf, nan = float("inf"), float("nan")
  g = lambda **kw: _capi.CnfFieldGrid(*[kw.get(k, v) for k, v in (("lo_x", -1.5), ("lo_y", -1.0), ("step_x", 0.5),
                                                                  ("step_y", 0.5), ("nx", 7), ("ny", 5), ("axis_x", 0),
                                                                  ("axis_y", 1))], -1, 1, None, None)
  refusals = (
    # the interaction's
    {"spec": None}, {"spec": _spec(kind=3)}, {"spec": _spec(kind=-1)}, {"spec": _spec(n_terms=0)}, {"spec": _spec(n_terms=5)},
    {"spec": _spec(amp=(1.0, 0.0))}, {"spec": _spec(amp=(nan, 1.0))}, {"spec": _spec(bw=(1.0, 0.0))},
    {"spec": _spec(bw=(1e-30, 1.0))}, {"spec": _spec(kind=2, amp=(0.0,))}, {"D": 0}, {"D": 15}, {"N": 1},
    {"N": (1 << 20) + 1}, {"R": 0}, {"R": 65},
    # kappa
    {"kappa": inf}, {"kappa": -inf}, {"kappa": nan},
    # the particle reference's
    {"drift": -1}, {"drift": 4}, {"drift": 1}, {"drift": 2}, {"drift": 3, "D": 2}, {"h": 0.0}, {"h": -0.01}, {"h": inf},
    {"h": nan}, {"var0": 0.0}, {"var0": inf}, {"sigma": -0.1}, {"sigma": nan}, {"sigma": inf}, {"a": inf}, {"a": nan},
    {"n_steps": -1}, {"n_steps": (1 << 30) + 1}, {"n_steps": 11}, {"first": -1}, {"S": 0}, {"S": 65}, {"snap": None},
    {"snap": (ctypes.c_int64 * 4)(0, 1, 1, 12)}, {"snap": (ctypes.c_int64 * 4)(-1, 1, 5, 12)},
    {"snap": (ctypes.c_int64 * 4)(0, 5, 1, 12)}, {"snap": (ctypes.c_int64 * 4)(0, 1, 5, 13)},
    {"grid": None}, {"grid": g(nx=0)}, {"grid": g(ny=0)}, {"grid": g(nx=1 << 13, ny=(1 << 11) + 1)}, {"grid": g(step_x=0.0)},
    {"grid": g(step_y=-0.5)}, {"grid": g(step_x=inf)}, {"grid": g(lo_x=nan)}, {"grid": g(axis_x=1)}, {"grid": g(axis_y=3)},
    {"grid": g(axis_x=-1)},
    # the buffers
    {"state": None}, {"sums": None}, {"ws": None}, {"wsb": nbytes.value - 8},
    # a stream element index that does not fit: (first + R N) particles of (n_steps + 1) D elements
    {"first": (1 << 62)}, {"first": (1 << 63) - 1}, {"n_steps": 1 << 30, "first": 1 << 32},
  )
  for bad in refusals:
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad
  # (a drift at another D is refused whatever else is asked for)
  assert call(drift=3, D=2, grid=None, hist=None) == _capi.CNF_ERR_INVALID


def test_python_entry_points_refuse_before_the_device(monkeypatch):
  from cnf_ot_amd import applications as app, solvers
  from cnf_ot_amd.distributed import Shard
  inf, nan = float("inf"), float("nan")
  quad = {"kind": "quadratic", "amplitudes": [1.0]}
  good = dict(dim=2, T=0.5, a=1.0, sigma=0.5, subtype="ou", interaction=quad, strength=2.0, times=[0.0, 0.1, 0.5],
              n_particles=64, replicas=2, h=0.01)
  for bad in ({"subtype": "vortex"}, {"dim": 0}, {"dim": 15}, {"subtype": "lorenz"}, {"subtype": "gradient", "dim": 3},
              {"times": [0.0, 0.105]}, {"times": [0.1, 0.1]}, {"times": [-0.1, 0.1]}, {"times": []},
              {"times": np.arange(65) * 0.01}, {"h": 0.0}, {"h": -0.01}, {"h": nan}, {"var0": 0.0}, {"var0": inf},
              {"sigma": -1.0}, {"sigma": nan}, {"a": inf}, {"strength": inf}, {"strength": nan},
              {"interaction": {"kind": "coulomb"}}, {"interaction": {"kind": "gaussian", "bandwidths": [0.0]}},
              {"interaction": {"kind": "quadratic", "amplitudes": [0.0]}},
              {"interaction": {"kind": "gaussian", "amplitudes": [1.0] * 5, "bandwidths": [1.0] * 5}},
              {"n_particles": 1}, {"n_particles": (1 << 20) + 1}, {"replicas": 0}, {"replicas": 65},
              {"x0": np.zeros((2, 63, 2))}, {"x0": np.zeros((64, 2))}, {"grid": ((-1, 1, -1, 1), 1)},
              {"grid": ((-1, 1, -1, 1), 8), "axes": (0, 0)}, {"grid": ((-1, 1, -1, 1), 8), "axes": (0, 2)},
              {"grid": ((1, -1, -1, 1), 8)}, {"seed": 0, "h": 1e-9, "T": 1e3, "times": [0.0]}):
    kw = dict(good, **bad)
    with pytest.raises(ValueError):
      app.mv_reference_particles(**kw)
  monkeypatch.setattr(app, "current_shard", lambda: Shard(0, 2))
  with pytest.raises(ValueError, match="all-gather"):
    app.mv_reference_particles(**good)
  monkeypatch.undo()

  # the solver: fp with an interaction kind only, in _fp_prelude's words
  ia = {"kind": "quadratic", "strength": 2.0, "amplitudes": [1.0], "bandwidths": [1.0]}
  fp_ou = {"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}}
  with pytest.raises(ValueError, match="defined for fp only"):
    solvers.evaluate_mv_reference(solvers.load_config(overrides={"interaction": ia}))
  with pytest.raises(ValueError, match="interaction kind"):
    solvers.evaluate_mv_reference(solvers.load_config(overrides=fp_ou))
  config = solvers.load_config(overrides=dict(fp_ou, interaction=ia))
  for kw in ({"n_particles": 63}, {"n_particles": 0}, {"times": [0.0, 0.0105], "h": 0.01}, {"replicas": 1},
             {"n_particles": (1 << 20) + 2}):
    with pytest.raises(ValueError):
      solvers.evaluate_mv_reference(config, **kw)
  with pytest.raises(ValueError, match="no figure settings"):
    solvers.evaluate_mv_reference(solvers.load_config(overrides=dict(fp_ou, interaction=ia, general={"type": "fp", "dim": 5})))
  with pytest.raises(ValueError):
    solvers.evaluate_mv_reference(solvers.load_config(overrides=dict(
      fp_ou, interaction={"kind": "gaussian", "strength": 1.0, "amplitudes": [1.0], "bandwidths": [-1.0]})))
  # the training term is still refused: this pull request adds the reference, not the term
  with pytest.raises(ValueError, match="fp_loss_fn"):
    solvers.bind_loss(config, None)
  assert "evaluate_mv_reference" in solvers.evaluate_interaction.__doc__
